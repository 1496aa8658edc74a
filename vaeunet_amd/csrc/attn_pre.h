// The attention gate's pre-activation s = BN(ug) + BN(ux) per channel
// (unet_parts.py:26: relu(g1 + x1)), from the raw conv outputs and the two
// BatchNorms' (scale, shift).  ONE text for every kernel that needs the ReLU
// mask s > 0 (psi forward, psi backward, the fused backward tail): they must
// agree on it bit for bit.  Contraction is OFF for this expression: left to
// the compiler, the same text became mul + add in the psi kernels and fused
// multiply-adds in the tail (its k pairs vectorise), and the masks then
// differed where |s| is within an ulp of zero -- a few elements per step at
// 8 x 512^2, enough to change a training run.
#pragma once
#include "common.h"

VU_DEV float attn_pre(float a, float wsg, float wtg, float b, float wsx, float wtx) {
#pragma clang fp contract(off)
  return a * wsg + wtg + b * wsx + wtx;
}
