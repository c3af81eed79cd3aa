/* The settings of mvg_augment_draw (rotmvgaze.h): one small host struct, read by the library during the call and
 * carried into the launch by value.  It lives in a header of its own, and rotmvgaze.h takes it as `const void *cfg`:
 * the set of structs rotmvgaze.h itself defines is pinned by the C-ABI tests.  Natural C alignment: ten floats at 0..40,
 * erase at 40, four bytes of padding, five doubles at 48..88.  The Python mirror is rot_mvgaze_amd/augment.py DRAW_CFG_DTYPE. */
#ifndef ROTMVGAZE_AUGMENT_DRAW_H
#define ROTMVGAZE_AUGMENT_DRAW_H

#include <stdint.h>

typedef struct mvg_augment_draw_cfg {
  float factor_lo[3];  /* brightness, contrast, saturation factor ranges; a disabled op is lo = hi = 1 */
  float factor_hi[3];
  float max_dx;        /* translate[0] * w and translate[1] * h (0: no translation) */
  float max_dy;
  float scale_lo;      /* RandomAffine's scale range (lo = hi = 1: none) */
  float scale_hi;
  int32_t erase;       /* 1: RandomMultiErasing follows (masks and grid are required) */
  double p;            /* ... its probability, */
  double prop_lo;      /* proportion range */
  double prop_hi;
  double dot_lo;       /* and dot-size range: 0 < dot_lo <= dot_hi, gmax = (int)(1.0 / dot_lo) */
  double dot_hi;
} mvg_augment_draw_cfg;

#endif
