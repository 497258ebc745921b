// The autotuner of the GEMM launchers (gemm.hip), host only: the trial timing of
// a candidate list, the table of choices per shape key and the scratch buffers
// the trial runs write to.
//
// By default the first call of a new shape times every applicable candidate on
// the caller's stream and caches the fastest, like a "find" step; ARTSBIR_TUNE=0
// (read at every new key) or a capturing stream takes the launcher's static
// choice instead.
//
// The tables as a text file (artsbir_tune_save / artsbir_tune_load): one line
// per key, a tag ("c" convolution keys, "w" weight-gradient keys), the key's
// fields in the order of its fields() as decimal integers and the choice,
// separated by single spaces and ended by '\n'; every "c" line in key order,
// then every "w" line.  Loading overwrites existing entries, stops at the first
// short or unknown line and skips retired choices without counting them.
// bench.py saves the file after a run and the profiled re-runs load it first, so
// rocprofv3 / PMC passes see only the launches of the steady-state step, no
// trial launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace artsbir {
namespace tune {

// One lock for every table: held while a new key is tuned, so the trial runs of
// two shapes never share the device.
inline std::mutex& mutex() {
  static std::mutex mu;
  return mu;
}

// grow-only device buffer of floats
struct Scratch {
  float* p = nullptr;
  size_t n = 0;
  bool reserve(size_t need) {
    if (need <= n) return true;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (hipMalloc(&p, need * sizeof(float)) != hipSuccess) return false;
    n = need;
    return true;
  }
};

// The fastest of cands on st: per candidate one untimed run(c) (the warm-up; false
// = c does not apply to the shape), then the minimum of three event-timed ones.
// The first candidate with the strictly smallest time wins; none if nothing ran.
template <typename Run>
int fastest(const std::vector<int>& cands, int none, hipStream_t st, Run run) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  // time the candidates on a quiet device: work queued on other streams (the
  // caller's overlapped weight gradients) would otherwise share the chip with
  // some trials and not others and make the choice noisy
  (void)hipDeviceSynchronize();
  int best = none;
  float best_ms = 1e30f;
  for (int c : cands) {
    if (!run(c)) continue;
    float ms = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
      (void)hipEventRecord(e0, st);
      run(c);
      (void)hipEventRecord(e1, st);
      (void)hipEventSynchronize(e1);
      float t = 0.f;
      (void)hipEventElapsedTime(&t, e0, e1);
      if (t < ms) ms = t;
    }
    if (ms < best_ms) { best_ms = ms; best = c; }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return best;
}

// Choice per shape key.  Key names its integer fields once, as
//   template <typename K> static auto fields(K& k) { return std::tie(k.a, k.b, ...); }
// which orders the keys and drives the file's writer and reader.
template <typename Key>
struct KeyLess {
  bool operator()(const Key& a, const Key& b) const { return Key::fields(a) < Key::fields(b); }
};

template <typename Key>
class Table {
 public:
  // the choice stored for key; for a new key fixed() if tuning is off or st is
  // capturing, else tuned(), stored
  template <typename Fixed, typename Tuned>
  int choice(const Key& key, hipStream_t st, Fixed fixed, Tuned tuned) {
    std::lock_guard<std::mutex> lk(mutex());
    auto it = map_.find(key);
    if (it != map_.end()) return it->second;
    const char* env = getenv("ARTSBIR_TUNE");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    const int c = ((env && atoi(env) == 0) || cs != hipStreamCaptureStatusNone) ? fixed() : tuned();
    map_[key] = c;
    return c;
  }

  // (the caller holds mutex())
  void write(FILE* f, char tag) const {
    for (const auto& kv : map_) {
      fputc(tag, f);
      std::apply([&](const auto&... v) { (fprintf(f, " %lld", (long long)v), ...); }, Key::fields(kv.first));
      fprintf(f, " %d\n", kv.second);
    }
  }

  // the rest of a line after its tag: -1 short line, 0 a retired choice
  // (skipped), 1 stored (the caller holds mutex())
  template <typename Retired>
  int read(FILE* f, Retired retired) {
    Key k;
    int c;
    bool ok = true;
    std::apply([&](auto&... v) { ((ok = ok && scan(f, v)), ...); }, Key::fields(k));
    if (!ok || fscanf(f, "%d", &c) != 1) return -1;
    if (retired(c)) return 0;
    map_[k] = c;
    return 1;
  }

 private:
  template <typename V>
  static bool scan(FILE* f, V& v) {
    long long t;
    if (fscanf(f, "%lld", &t) != 1) return false;
    v = (V)t;
    return true;
  }
  std::map<Key, int, KeyLess<Key>> map_;
};

}  // namespace tune
}  // namespace artsbir
