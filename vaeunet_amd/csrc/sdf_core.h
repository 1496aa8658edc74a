// Per-pixel steps of the signed distance map (sdf.hip, DESIGN.md §4.13;
// definitions: include/vaeunet.h) that edt_core.h does not already have.
//
//   sdf_pack / sdf_gf / sdf_gb   the column pass leaves two vertical distances in
//                                one int32 word: to the nearest foreground row of
//                                the column in the low half, to the nearest
//                                background row in the high half.  Both are
//                                <= EDT_NONE = 32768 and fit 16 bits each.
//   sdf_is_fg                    a pixel is foreground when its own distance to
//                                the foreground is 0: the row pass needs no second
//                                look at the input
//   sdf_opposite                 the row a pixel searches: the distances to the
//                                class it does not belong to
//   sdf_signed                   the sign: + outside, - inside
//   sdf_phi                      s2 -> phi, rounded once from fp64, then the clip
//
// No HIP dependency, as edt_core.h: a host program can include this file and run
// both passes serially (tests/test_sdf_core.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include "edt_core.h"

VU_EDT_HD int32_t sdf_pack(int32_t gf, int32_t gb) { return (int32_t)((uint32_t)gf | ((uint32_t)gb << 16)); }
VU_EDT_HD uint16_t sdf_gf(int32_t w) { return (uint16_t)((uint32_t)w & 0xffffu); }
VU_EDT_HD uint16_t sdf_gb(int32_t w) { return (uint16_t)((uint32_t)w >> 16); }

VU_EDT_HD bool sdf_is_fg(uint16_t gf) { return gf == 0; }

// rows of the vertical distances to the foreground / to the background, W each
VU_EDT_HD const uint16_t* sdf_opposite(const uint16_t* to_fg, const uint16_t* to_bg, bool fg) {
  return fg ? to_bg : to_fg;
}

// d2: the squared distance to the nearest pixel of the other class (>= 1 on a plane that has both)
VU_EDT_HD int32_t sdf_signed(int32_t d2, bool fg) { return fg ? -d2 : d2; }

// clip > 0, +inf for none
VU_EDT_HD float sdf_phi(int32_t s2, float clip) {
  float phi = 0.f;
  if (s2 > 0) phi = (float)sqrt((double)s2);
  else if (s2 < 0) phi = (float)(1.0 - sqrt(-(double)s2));
  phi = phi > clip ? clip : phi;
  return phi < -clip ? -clip : phi;
}
