"""Shared by the parity tests of the register-staged GEMM family of csrc/gemm.hip (test
infrastructure): test_regstaged_gpu.py and test_regstaged_inputs.py.  The kernels are
conv_gemm_kernel<T,128,64|128> (forward, data gradient, dense NT) and
wgrad_kernel<T,64|128,128> (weight gradient, dense TN), T = f32 or bf16.

Reference.  float64 on the CPU from the operands as stored (bf16-rounded for bf16).  The
im2col matrix Xcol [M][K], k = (r, s, ci), comes from F.unfold of the (affine, ReLU'd)
input in float64; every output is the float64 sum of its terms: the K products of a
convolution (M products of a weight gradient) plus the bias, the residual
(_convref.residual) and the previous content of an accumulated output.  ReLU is applied
to the sum.  test_regstaged_inputs.py holds Xcol's own ordering to torch's float64
conv2d / conv2d_input / conv2d_weight.

Bars (none measured on the code under test).  An f32 output is held to _convref.seg_sums's
bar along its reduction axis,
    |out - ref64| <= min(max(8 e_seq, 8 2^-24 sum |term|), n 2^-24 sum |term|),
e_seq the error of a float32 numpy.cumsum of the float64 terms; a bf16-stored output gets
2^-8 |ref64| on top (one rounding of the f32 result, _tail.check_bf16's form).  The BN sums
(replica slots added in float64) are held to seg_sums over the float64 y and y^2 (bias
included), per segment and channel.  The bars are computed eight output columns at a time
and cached with the problem.

Affine loaders use dyadic data (x a multiple of 1/8 in [-4, 4], scale in {1/2, 1, 2},
shift a multiple of 1/8 in [-2, 2]) so that x * scale + shift is exact in bf16 and f32,
fused or not, and needs no allowance; some shifts are positive, so a shift leaking into
the zero padding shows under ReLU.

The offset caps of launch_wgrad_tile (2^22 pixels, 2^30 bytes per block) are reached by no
test-sized shape and are not covered here."""
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

import _convref as cr

BF = torch.bfloat16
DT = {"f32": torch.float32, "bf16": BF}
EPC = {"f32": 4, "bf16": 8}   # elements per 16-byte chunk
BK = {"f32": 32, "bf16": 64}  # the K-step (eight chunks)


# ---------------------------------------------------------------------------
# the launchers' arithmetic, restated (gemm.hip: conv_gemm_kernel's load_tiles and store
# loop, launch_conv_old, launch_wgrad_old, launch_wgrad_tile)
def decoder(C, dt):
    """the tap decoder conv_gemm_kernel takes for C input channels"""
    if C % BK[dt] == 0:
        return "uniform"
    if C < BK[dt] and BK[dt] % C == 0:
        return "divides"
    return "generic"


def conv_kernel(dt, Co):
    return f"conv_gemm_kernel<{dt},128,{64 if Co <= 64 else 128}>"


def wgrad_kernel(dt, Co):
    return f"wgrad_kernel<{dt},{64 if Co <= 64 else 128},128>"


def store_paths(Co, ldy, out_f32, acc):
    """the store forms the eight-column chunks of a row take"""
    paths = set()
    for gn in range(0, Co, 8):
        nv = min(8, Co - gn)
        vec = nv == 8 and ldy % (4 if out_f32 else 8) == 0
        paths.add(("acc-" if acc else "") + ("vec" if vec else "scalar-tail" if nv < 8 else "scalar-ld"))
    return paths


def wgrad_splits(dt, M, Co, K):
    """(splits, m_per_split) of launch_wgrad_tile below its offset caps"""
    bm = 64 if Co <= 64 else 128
    tiles = -(-Co // bm) * -(-K // 128)
    ksteps = -(-M // BK[dt])
    splits = max(1, min(-(-1024 // tiles), (ksteps + 7) // 8))
    per = -(-ksteps // splits)
    return -(-ksteps // per), per * BK[dt]


# ---------------------------------------------------------------------------
# cases
class Conv(NamedTuple):
    """api: fwd (artsbir_conv2d_fwd), seg (_fwd_seg), act (_fwd_act), dgrad (artsbir_conv2d_dgrad), nt
    (artsbir_gemm_nt).  geo: (N, H, W, C, Cout, R, S, stride, pad) of the entry point's descriptor; for nt
    (M, N, K, lda - K, 0, ...) as (M, 1, 1, K, N, 1, 1, 1, 0) with the row gap in opts.
    opts: stats bias relu res1 res2 f32out acc aff0 aff1 seg3 ld+8 ld+3 lda+8 lda+16"""
    api: str
    dt: str
    geo: tuple
    opts: tuple = ()

    @property
    def id(self):
        return f"{self.api}-{self.dt}-" + "x".join(map(str, self.geo)) + "".join("-" + o for o in self.opts)


class Wgrad(NamedTuple):
    """api: conv (artsbir_conv2d_wgrad) or tn (artsbir_gemm_tn, geo (M, 1, 1, K, N, 1, 1, 1, 0));
    opts: aff0 aff1 ldd+8 ldd+16 ldx+8"""
    api: str
    dt: str
    geo: tuple
    opts: tuple = ()

    @property
    def id(self):
        return f"w{self.api}-{self.dt}-" + "x".join(map(str, self.geo)) + "".join("-" + o for o in self.opts)


# Every decoder x dtype x tile with the plain epilogue and statistics.  Per row: the geometry, the
# decoder it must reach in f32 and in bf16, the tile.  The filter geometries of the issue are spread
# over the rows: 3x3 (stride 1, stride 2 on 9x7), 1x1 stride 2, 5x5 pad 2, 1x7, 3x1, 4x8 (32 taps,
# bit 31 of rmask), K = 216 (no multiple of either K-step); M is one partial tile (< 128) or several
# tiles with Ho*Wo not dividing 128 and a partial last one.
DECODER_ROWS = [
    # N  H   W   C   Co  R  S st pd    f32        bf16     tile
    ((3, 9, 7, 8, 64, 3, 3, 2, 1), "divides", "divides", 64),      # M 60
    ((2, 10, 13, 8, 72, 4, 8, 1, 1), "divides", "divides", 128),   # M 144 (9x8 maps), K 256
    ((5, 7, 5, 16, 5, 5, 5, 1, 2), "divides", "divides", 64),      # M 175, K 400
    ((2, 6, 9, 16, 136, 1, 7, 1, 0), "divides", "divides", 128),   # M 36 (6x3 maps), K 112
    ((2, 9, 7, 24, 20, 5, 5, 1, 2), "generic", "generic", 64),     # M 126, K 600
    ((3, 9, 7, 24, 72, 3, 3, 2, 1), "generic", "generic", 128),    # M 60, K 216
    ((5, 11, 9, 32, 64, 1, 1, 2, 0), "uniform", "divides", 64),    # M 150 (6x5 maps), K 32
    ((5, 6, 5, 32, 136, 3, 1, 1, 1), "uniform", "divides", 128),   # M 210 (6x7 maps), K 96
    ((2, 10, 13, 40, 20, 4, 8, 1, 1), "generic", "generic", 64),   # M 144, K 1280
    ((3, 7, 5, 40, 72, 3, 3, 1, 1), "generic", "generic", 128),    # M 105, K 360
    ((3, 9, 7, 48, 64, 3, 3, 2, 1), "generic", "generic", 64),     # M 60, K 432
    ((4, 6, 9, 48, 136, 1, 7, 1, 0), "generic", "generic", 128),   # M 72, K 336
    ((5, 7, 5, 64, 64, 3, 3, 1, 1), "uniform", "uniform", 64),     # M 175, K 576
    ((1, 9, 7, 64, 136, 5, 5, 1, 2), "uniform", "uniform", 128),   # M 63, K 1600
    ((2, 6, 5, 64, 72, 3, 1, 1, 1), "uniform", "uniform", 128),    # M 84 (6x7 maps), K 192
    ((3, 7, 5, 96, 5, 3, 3, 1, 1), "uniform", "generic", 64),      # M 105, K 864
    ((5, 11, 9, 96, 72, 1, 1, 2, 0), "uniform", "generic", 128),   # M 150, K 96
]

# the two shapes every epilogue runs on: uniform taps and the generic decoder in both dtypes
SHAPE_U = (3, 7, 5, 64, None, 3, 3, 1, 1)   # M 105, K 576
SHAPE_G = (3, 9, 7, 24, None, 3, 3, 1, 1)   # M 189 (two tiles, the last partial), K 216
SHAPE_DEC = {"U": ("uniform", "uniform"), "G": ("generic", "generic")}

# artsbir_conv2d_fwd: (opts, Cout, the store forms it must reach)
FWD_EPILOGUES = [
    (("bias",), 20, {"scalar-ld", "scalar-tail"}),
    (("bias", "ld+8"), 72, {"vec"}),
    (("stats", "ld+3"), 20, {"scalar-ld", "scalar-tail"}),
    (("ld+3",), 64, {"scalar-ld"}),
    (("stats", "bias"), 136, {"vec"}),
    (("f32out",), 20, {"vec", "scalar-tail"}),
    (("f32out", "bias"), 5, {"scalar-tail"}),
    (("f32out", "ld+3", "stats"), 72, {"scalar-ld"}),
    (("f32out", "acc"), 64, {"acc-vec"}),
    (("f32out", "acc", "ld+8"), 20, {"acc-vec", "acc-scalar-tail"}),
    (("f32out", "acc", "bias"), 5, {"acc-scalar-tail"}),
    (("f32out", "acc", "ld+3"), 72, {"acc-scalar-ld"}),
    (("aff0", "stats"), 64, {"vec"}),
    (("aff1", "stats"), 20, {"scalar-ld", "scalar-tail"}),
    (("aff1", "bias", "f32out"), 72, {"vec"}),
]
ACT_EPILOGUES = [(("bias", "relu"), 20), (("bias", "relu", "res1"), 72), (("bias", "res1"), 64)]
SEG_COUT = {"U": 72, "G": 64}

# artsbir_conv2d_dgrad (N, H, W, Cin, Cout, R, S, 1, pad) + res_mode; the kernel's input channels are
# Cout: 40 generic / generic, 64 uniform / uniform, 24 generic / generic, 32 uniform / divides,
# 96 uniform / generic.  Mode 2 on 8x12 (H/2 != W/2), M = 288 (no multiple of 128).
DGRAD_ROWS = [
    ((3, 8, 12, 24, 40, 3, 3, 1, 1), "res2"),
    ((3, 8, 12, 72, 64, 1, 1, 1, 0), "res2"),
    ((2, 7, 5, 40, 24, 3, 3, 1, 1), "res1"),
    ((2, 7, 5, 136, 32, 1, 1, 1, 0), "res1"),
    ((2, 7, 5, 8, 96, 3, 3, 1, 1), None),
    ((3, 8, 12, 16, 64, 1, 1, 1, 0), None),
]

# artsbir_gemm_nt (M, N, K, opts): lda > K with NaN in the gaps, ldc > N
NT_ROWS = [
    (37, 20, 24, ("lda+8", "ld+3", "bias", "stats")),
    (300, 72, 40, ("lda+16", "ld+8", "bias", "stats")),
    (150, 40, 2048, ("lda+8", "ld+3", "bias", "stats")),
    (600, 64, 40, ("lda+8", "f32out", "acc")),
    (100, 5, 2048, ("lda+8", "f32out")),
]


def _conv_cases():
    cases = []
    for dt in ("f32", "bf16"):
        for geo, *_ in DECODER_ROWS:
            cases.append(Conv("fwd", dt, geo, ("stats",)))
        for name, shape in (("U", SHAPE_U), ("G", SHAPE_G)):
            with_co = lambda co: shape[:4] + (co,) + shape[5:]  # noqa: E731
            for opts, co, _ in FWD_EPILOGUES:
                cases.append(Conv("fwd", dt, with_co(co), opts))
            for opts, co in ACT_EPILOGUES:
                cases.append(Conv("act", dt, with_co(co), opts))
            cases.append(Conv("seg", dt, with_co(SEG_COUT[name]), ("stats", "seg3")))
        for geo, res in DGRAD_ROWS:
            cases.append(Conv("dgrad", dt, geo, (res,) if res else ()))
        for M, N, K, opts in NT_ROWS:
            cases.append(Conv("nt", dt, (M, 1, 1, K, N, 1, 1, 1, 0), opts))
    return cases


CONV_CASES = _conv_cases()

# wgrad_kernel: (geo, opts, what the row is for)
WGRAD_ROWS = [
    ((37, 1, 1, 8, 8, 3, 3, 1, 1), ()),      # 1x1 maps: every pixel wraps a row and an image; M 37; K 72
    ((1, 1, 1, 24, 64, 3, 3, 1, 1), ()),     # M 1; K 216
    ((11, 2, 2, 8, 72, 3, 3, 1, 1), ()),     # 2x2 maps: a unit spans images; M 44 (< BK in bf16)
    ((5, 3, 5, 128, 8, 3, 3, 1, 1), ()),     # 3x5 maps, M 75, K 1152 (nine K tiles)
    ((3, 7, 5, 128, 136, 3, 3, 1, 1), ()),   # K 1152 on the 128-row tile, M 105
    ((17, 7, 5, 24, 136, 3, 3, 1, 1), ()),   # M 595: f32 m_per_split 224 (35 and 5 do not divide it)
    ((30, 7, 5, 8, 64, 5, 5, 1, 2), ()),     # M 1050: bf16 m_per_split 384; K 200
    ((9, 9, 14, 8, 8, 3, 3, 1, 1), ()),      # 9x14 maps, M 1134: f32 256 x 5, bf16 384 x 3, last partial
    ((7, 9, 7, 8, 72, 3, 3, 2, 1), ()),      # stride 2 on 9x7 (5x4 maps), M 140
    ((6, 9, 7, 24, 64, 1, 1, 2, 0), ()),     # 1x1 stride 2: the non-dense form, K 24
    ((4, 7, 5, 24, 64, 3, 3, 1, 1), ("aff0",)),
    ((4, 7, 5, 24, 64, 3, 3, 1, 1), ("aff1",)),
    ((2, 3, 5, 8, 72, 3, 3, 1, 1), ("aff1",)),
]
TN_ROWS = [
    (37, 8, 72, ("ldd+8", "ldx+8")),
    (600, 72, 200, ("ldd+16", "ldx+8")),
    (600, 64, 24, ("ldd+8", "ldx+8")),
    (1051, 136, 40, ("ldd+8", "ldx+8")),
]


def _wgrad_cases():
    cases = []
    for dt in ("f32", "bf16"):
        cases += [Wgrad("conv", dt, geo, opts) for geo, opts in WGRAD_ROWS]
        cases += [Wgrad("tn", dt, (M, 1, 1, K, N, 1, 1, 1, 0), opts) for M, N, K, opts in TN_ROWS]
    return cases


WGRAD_CASES = _wgrad_cases()


def _extra(opts, prefix):
    for o in opts:
        if o.startswith(prefix + "+"):
            return int(o[len(prefix) + 1:])
    return 0


# ---------------------------------------------------------------------------
# problems
def _stored(x, dt):
    """float64 values as stored in dt"""
    return x.to(DT[dt]).double()


def _seed(case):
    return sum((i + 1) * v for i, v in enumerate(case.geo)) + 7919 * len(case.opts) + sum(map(ord, case.id)) % 9973


def _affine(opts, C, g):
    """(scale, shift, relu) of the dyadic affine loader, or None"""
    if "aff0" not in opts and "aff1" not in opts:
        return None
    sc = torch.tensor([0.5, 1.0, 2.0]).double()[torch.randint(0, 3, (C,), generator=g)]
    sh = torch.randint(-16, 17, (C,), generator=g).double() / 8
    sh[0], sh[C - 1] = 0.75, -0.5  # a positive and a negative shift whatever the draw
    return sc, sh, int("aff1" in opts)


def _input(shape, dt, aff, g, zones=None):
    """the stored input NCHW and what the loader makes of it (float64)"""
    if aff is not None:
        x = torch.randint(-32, 33, shape, generator=g).double() / 8
        sc, sh, relu = aff
        a = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        return x, torch.relu(a) if relu else a
    x = torch.randn(shape, generator=g).double()
    if zones is not None:
        x = x + 0.5 * zones.view(-1, 1, 1, 1)
    x = _stored(x, dt)
    return x, x


def _xcol(a, R, S, stride, pad):
    """im2col [M][K] of a [N][C][H][W], k = (r, s, ci), and the in-bounds flag of every (m, tap)"""
    N, C = a.shape[:2]
    cols = F.unfold(a, (R, S), padding=pad, stride=stride)                      # [N][C*R*S][L], (c, r, s)
    L = cols.shape[-1]
    xcol = cols.view(N, C, R * S, L).permute(0, 3, 2, 1).reshape(N * L, R * S * C)
    ones = F.unfold(torch.ones(1, 1, *a.shape[2:], dtype=a.dtype), (R, S), padding=pad, stride=stride)
    valid = ones.view(R * S, L).t().repeat(N, 1) > 0                            # [M][taps]
    return xcol.contiguous(), valid


class ConvProblem:
    """inputs, float64 result and bars of one Conv case.  Everything the kernel reads is in the form it is
    stored: x2d [rows][C] (NHWC pixels, or the dense A), w2d [Cout][K], bias, res2d, prev, scale / shift"""

    def __init__(self, case):
        self.case = case
        api, dt, geo, opts = case
        g = torch.Generator().manual_seed(_seed(case))
        N, H, W, C, Co, R, S, stride, pad = geo
        self.desc_geo = geo
        if api == "dgrad":  # a convolution of dy [N][H][W][Cout] with wd [Cin][R][S][Cout], padding R-1-pad
            C, Co, pad = Co, C, R - 1 - pad
        self.C, self.Co, self.R, self.S, self.stride, self.pad = C, Co, R, S, stride, pad
        self.K = R * S * C
        self.nseg = 3 if "seg3" in opts else 1
        self.aff = _affine(opts, C, g)
        zones = (torch.arange(N) * self.nseg // N).double() if self.nseg > 1 else None
        x, a = _input((N, C, H, W), dt, self.aff, g, zones)
        self.x2d = cr.flat(x)
        self.xcol, self.valid = _xcol(a, R, S, stride, pad)
        self.M = self.xcol.shape[0]
        self.Ho = (H + 2 * pad - R) // stride + 1
        self.Wo = (W + 2 * pad - S) // stride + 1
        self.w2d = _stored(torch.randn(Co, self.K, generator=g) / self.K ** 0.5, dt)
        self.ldy = Co + _extra(opts, "ld")
        self.lda = C + _extra(opts, "lda")
        self.out_f32 = int("f32out" in opts)
        self.acc = int("acc" in opts)
        self.relu = int("relu" in opts)
        self.out_dt = "f32" if self.out_f32 else dt
        self.bias = torch.randn(Co, generator=g).float().double() if "bias" in opts else None
        self.res_mode = 1 if "res1" in opts else 2 if "res2" in opts else 0
        self.res2d = self.res_term = None
        if self.res_mode:
            rs = (N, Co, self.Ho, self.Wo) if self.res_mode == 1 else (N, Co, self.Ho // 2, self.Wo // 2)
            res = _stored(torch.randn(rs, generator=g), dt)
            self.res2d = cr.flat(res)
            self.res_term = cr.flat(cr.residual(res, self.res_mode))
        self.prev = torch.randn(self.M, Co, generator=g).float().double() if self.acc else None
        self._bars()

    def extras(self, n0, n1):
        """the terms of columns n0..n1 besides the K products: [E][M][n1-n0]"""
        e = []
        if self.bias is not None:
            e.append(self.bias[n0:n1].expand(self.M, -1))
        if self.res_term is not None:
            e.append(self.res_term[:, n0:n1])
        if self.prev is not None:
            e.append(self.prev[:, n0:n1])
        return e

    def _bars(self):
        M, Co, K = self.M, self.Co, self.K
        self.pre = torch.empty(M, Co, dtype=torch.float64)   # the float64 sum before the ReLU
        self.bar = torch.empty(M, Co, dtype=torch.float64)
        xt = self.xcol.t().contiguous()
        for n0 in range(0, Co, 8):
            n1 = min(n0 + 8, Co)
            t = xt[:, :, None] * self.w2d[n0:n1].t()[:, None, :]            # [K][M][8]
            t = torch.cat([t] + [e[None] for e in self.extras(n0, n1)], 0)
            ref, bar = cr.seg_sums(t.reshape(t.shape[0], -1), 1)
            self.pre[:, n0:n1] = torch.from_numpy(ref[0]).view(M, n1 - n0)
            self.bar[:, n0:n1] = torch.from_numpy(bar[0]).view(M, n1 - n0)
        self.ref = torch.relu(self.pre) if self.relu else self.pre
        if self.out_dt == "bf16":
            self.bar = self.bar + 2.0 ** -8 * self.ref.abs()
        # the statistics' terms: the convolution and the bias (no entry point adds more under stats)
        self.y_stats = None
        if "stats" in self.case.opts:
            assert self.res_term is None and self.prev is None and not self.relu
            self.y_stats = self.pre

    def torch_ref(self):
        """the same result from torch's own float64 convolution (the check of Xcol's ordering)"""
        N, H, W = self.desc_geo[:3]
        x = self.x2d.view(N, H, W, self.C).permute(0, 3, 1, 2)
        if self.aff is not None:
            sc, sh, relu = self.aff
            x = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
            x = torch.relu(x) if relu else x
        if self.case.api == "dgrad":
            dN, dH, dW, Ci, Cout, R, S, _, dpad = self.desc_geo
            w = self.w2d.view(Ci, R, S, Cout).flip(1, 2).permute(3, 0, 1, 2)   # [Cout][Cin][R][S]
            y = torch.nn.grad.conv2d_input((dN, Ci, dH, dW), w, x, stride=1, padding=dpad)
        else:
            w = self.w2d.view(self.Co, self.R, self.S, self.C).permute(0, 3, 1, 2)
            y = F.conv2d(x, w, stride=self.stride, padding=self.pad)
        y = cr.flat(y)
        for e in self.extras(0, self.Co):
            y = y + e
        return torch.relu(y) if self.relu else y

    def stats_sums(self):
        """[(name, terms [M][Cout])] of the statistics"""
        return [("sum y", self.y_stats), ("sum y^2", self.y_stats * self.y_stats)]

    def sensitivity(self):
        """min over the chunk positions g (EPC consecutive k) of the largest move, in units of 4 bars, of a
        checked output when (drop) chunk g is left out of the reduction, (tap) chunk g reads the input of
        the neighbouring filter tap, (seg) chunk g's share of a segment's sum y is credited to the
        neighbouring segment.  None where the change does not exist (one tap, one segment)."""
        epc = EPC[self.case.dt]
        M, Co, K = self.M, self.Co, self.K
        G, taps, cg = K // epc, self.R * self.S, self.C // epc
        xg = self.xcol.view(M, G, epc)
        wg = self.w2d.view(Co, G, epc)
        act = torch.relu if self.relu else (lambda v: v)
        four = (4 * self.bar).clamp_min(1e-300)  # a bar of zero (an all-padding pixel): the output is exactly zero

        def moved(delta):  # [G][M][Co] -> [G]
            return ((act(self.pre + delta) - self.ref).abs() / four).amax((1, 2))

        drop = torch.einsum("mge,nge->gmn", xg, wg)
        out = {"drop": moved(-drop), "tap": None, "seg": None}
        if taps > 1:
            nb = torch.tensor(list(range(1, taps)) + [taps - 2])
            xn = self.xcol.view(M, taps, cg, epc)[:, nb].reshape(M, G, epc)
            out["tap"] = moved(torch.einsum("mge,nge->gmn", xn - xg, wg))
        if self.y_stats is not None:
            _, sbar = cr.seg_sums(self.y_stats, self.nseg)                    # [nseg][Co]
            share = drop.view(G, self.nseg, M // self.nseg, Co).sum(2).abs()  # [G][nseg][Co]
            sbar = torch.from_numpy(sbar)
            s_drop = (share / (4 * sbar)).amax((1, 2))
            out["drop"] = torch.maximum(out["drop"], s_drop)
            if self.nseg > 1:  # the share of segment s lands in segment s +- 1: both sums move by it
                tight = torch.minimum(sbar, torch.minimum(sbar.roll(1, 0), sbar.roll(-1, 0)))
                out["seg"] = (share / (4 * tight)).amax((1, 2))
        return {k: (None if v is None else float(v.min())) for k, v in out.items()}


class WgradProblem:
    """inputs, float64 result and bars of one Wgrad case: dw [Cout][K] = prev + sum_m dy[m][co] Xcol[m][k]"""

    def __init__(self, case):
        self.case = case
        api, dt, geo, opts = case
        g = torch.Generator().manual_seed(_seed(case))
        N, H, W, C, Co, R, S, stride, pad = geo
        self.C, self.Co, self.R, self.S, self.stride, self.pad = C, Co, R, S, stride, pad
        self.K = R * S * C
        self.aff = _affine(opts, C, g)
        x, a = _input((N, C, H, W), dt, self.aff, g)
        self.x2d = cr.flat(x)
        self.xcol, self.valid = _xcol(a, R, S, stride, pad)
        self.M = self.xcol.shape[0]
        self.Ho = (H + 2 * pad - R) // stride + 1
        self.Wo = (W + 2 * pad - S) // stride + 1
        self.dy = _stored(torch.randn(self.M, Co, generator=g), dt)
        self.prev = torch.randn(Co, self.K, generator=g).float().double()
        self.ldd = Co + _extra(opts, "ldd")
        self.ldx = C + _extra(opts, "ldx")
        self.splits, self.m_per_split = wgrad_splits(dt, self.M, Co, self.K)
        self.ref = torch.empty(Co, self.K, dtype=torch.float64)
        self.bar = torch.empty(Co, self.K, dtype=torch.float64)
        for c0 in range(0, Co, 8):
            t = self.dy[:, c0:c0 + 8, None] * self.xcol[:, None, :]              # [M][8][K]
            t = torch.cat([self.prev[None, c0:c0 + 8], t], 0)
            ref, bar = cr.seg_sums(t.reshape(t.shape[0], -1), 1)
            self.ref[c0:c0 + 8] = torch.from_numpy(ref[0]).view(-1, self.K)
            self.bar[c0:c0 + 8] = torch.from_numpy(bar[0]).view(-1, self.K)

    def torch_ref(self):
        """prev + torch's float64 conv2d_weight, as [Cout][R][S][C]"""
        N, H, W = self.case.geo[:3]
        x = self.x2d.view(N, H, W, self.C).permute(0, 3, 1, 2)
        if self.aff is not None:
            sc, sh, relu = self.aff
            x = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
            x = torch.relu(x) if relu else x
        dy = self.dy.view(N, self.Ho, self.Wo, self.Co).permute(0, 3, 1, 2)
        dw = torch.nn.grad.conv2d_weight(x, (self.Co, self.C, self.R, self.S), dy, stride=self.stride,
                                         padding=self.pad)
        return self.prev + dw.permute(0, 2, 3, 1).reshape(self.Co, self.K)

    def sensitivity(self):
        """min over the loader positions that carry data of the largest move of a dw element, in units of
        4 bars, when (drop) one unit of EPC pixels of one filter tap is left out, (tap) that unit reads the
        neighbouring tap's input, (whole) one tap is left out for every pixel.  A (unit, tap) whose pixels
        all lie in the padding carries no data: leaving it out changes nothing, and it is not counted."""
        epc = EPC[self.case.dt]
        M, Co, C = self.M, self.Co, self.C
        taps = self.R * self.S
        U = -(-M // epc)
        padm = U * epc - M
        dy = torch.cat([self.dy, torch.zeros(padm, Co, dtype=torch.float64)]).view(U, epc, Co)
        xc = torch.cat([self.xcol, torch.zeros(padm, self.K, dtype=torch.float64)]).view(U, epc, taps, C)
        live = torch.cat([self.valid, torch.zeros(padm, taps, dtype=torch.bool)]).view(U, epc, taps).any(1)
        four = (4 * self.bar).clamp_min(1e-300).view(Co, taps, C)

        def moved(delta):  # [U][Co][taps][C] -> [U][taps]
            return (delta.abs() / four).amax((1, 3))

        drop = torch.einsum("ueo,uetc->uotc", dy, xc)
        r_drop = moved(drop)
        out = {"drop": float(r_drop[live].min()), "tap": None,
               "whole": float((drop.sum(0).abs() / four).amax((0, 2))[live.any(0)].min())}
        if taps > 1:
            nb = torch.tensor(list(range(1, taps)) + [taps - 2])
            r_tap = moved(torch.einsum("ueo,uetc->uotc", dy, xc[:, :, nb] - xc))
            out["tap"] = float(r_tap[live | live[:, nb]].min())
        return out


@functools.lru_cache(maxsize=2)
def problem(case):
    return (ConvProblem if isinstance(case, Conv) else WgradProblem)(case)
