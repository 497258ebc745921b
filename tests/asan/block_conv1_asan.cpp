// Host-side AddressSanitizer check of artsbir_block_out_conv1x1_fwd's argument
// checks, linked against libartsbir_hip_asan.so like capi_asan.cpp: every call
// below is rejected before any kernel launch or device access, so it runs on a
// machine without a GPU.  Prints "asan block_conv1 ok" and exits 0.
#include <stdio.h>
#include <string.h>

#include "../../include/artsbir.h"

static int fails = 0;
#define EXPECT(c)                                                 \
  do {                                                            \
    if (!(c)) { fprintf(stderr, "FAILED: %s (line %d)\n", #c, __LINE__); ++fails; } \
  } while (0)

int main() {
  float f[4] = {0, 0, 0, 0};  // stands in for every operand: no call below reads it
  void* p = f;
  const artsbir_conv_desc ok = {ARTSBIR_DT_BF16, 6, 8, 8, 256, 64, 1, 1, 1, 0};
  artsbir_conv_desc d;

  EXPECT(artsbir_block_out_conv1x1_fwd(NULL, p, f, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "null descriptor") != NULL);
  d = ok; d.R = d.S = 3; d.pad = 1;  // not a 1x1 conv
  EXPECT(artsbir_block_out_conv1x1_fwd(&d, p, f, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "1x1") != NULL);
  d = ok; d.stride = 2;
  EXPECT(artsbir_block_out_conv1x1_fwd(&d, p, f, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  d = ok; d.C = 12;  // not a multiple of 8
  EXPECT(artsbir_block_out_conv1x1_fwd(&d, p, f, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "multiple of 8") != NULL);
  d = ok; d.Cout = 0;
  EXPECT(artsbir_block_out_conv1x1_fwd(&d, p, f, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  // segments that do not divide the batch, no segments
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, NULL, NULL, p, p, 4, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "segments") != NULL);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, NULL, NULL, p, p, 0, p, NULL, p, f, NULL) == -1);
  // null operands: y3, bn3, w, out, y1; neither identity nor downsample; downsample without its BN
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, NULL, f, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "null operand") != NULL);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, NULL, NULL, NULL, p, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, NULL, NULL, p, NULL, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, NULL, NULL, p, p, 3, NULL, NULL, p, f, NULL) == -1);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, NULL, NULL, p, p, 3, p, NULL, NULL, f, NULL) == -1);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, NULL, NULL, NULL, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "identity") != NULL);
  EXPECT(artsbir_block_out_conv1x1_fwd(&ok, p, f, p, NULL, NULL, p, 3, p, NULL, p, f, NULL) == -1);
  EXPECT(strstr(artsbir_last_error(), "BN parameter block") != NULL);

  if (fails) return 1;
  printf("asan block_conv1 ok\n");
  return 0;
}
