// One element of the BatchNorm(+ReLU) backward apply: the gradient of the BN
// input x from the output gradient dz, the forward (scale, shift, mean) and
// the three apply coefficients of vu_bn_bwd_reduce / vu_bn_bwd_finish.  ONE
// text for bn_bwd_apply_kernel (bn.hip), which stores the result, and for the
// image weight gradient (conv_image_wgrad.hip), which feeds it to its MFMAs
// without storing it: both must form the same bits, the ReLU mask included.
// Contraction is OFF so that neither caller's surroundings can change it (as
// written nothing here contracts: the product is fmaf's addend).
#pragma once
#include "common.h"

VU_DEV float bn_bwd_elem(float xv, float dz, int relu, float sc, float sf, float mu, float k1, float k2,
                         float k3) {
#pragma clang fp contract(off)
  if (relu && !(fmaf(xv, sc, sf) > 0.f)) dz = 0.f;
  return fmaf(k1, dz, k2 * (xv - mu)) + k3;
}
