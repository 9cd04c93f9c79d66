// What wgrad.hip (tap-staged kernels, dispatch, slab sum) calls in wgrad_patch.hip (patch-staged kernels).  Not exported.
#pragma once
#include "adn_common.h"

// Eligibility + plan of the patch-staged kernel of d->geom: false = the layer takes the tap-staged plan.  Else `nsplit`
// pixel splits, each an f32 slab of `out_elems` (summed by the caller when nsplit > 1).  `d` has passed validation.
bool adn_wgrad_patch_plan(const AdnWgradDesc* d, int* nsplit, int64_t* out_elems);
// The launch of that plan: writes d->workspace (nsplit > 1) or d->dw.
int adn_wgrad_patch_launch(const AdnWgradDesc* d, int nsplit, int64_t out_elems, void* stream);
// n <= 4 k4 problems in one launch; nsplit[k] pixel splits and the slab (or, unsplit, dW) base out[k] per problem
int adn_wgrad_k4p_batch_launch(const AdnWgradDesc* descs, int n, const int* nsplit, float* const* out, void* stream);
