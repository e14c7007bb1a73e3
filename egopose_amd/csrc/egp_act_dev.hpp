// egp_act_dev.hpp -- the activations of the reference's MLPs (models/mlp.py:12-17: tanh, relu, sigmoid) and their derivatives
// as functions of the activation's OUTPUT, in one place: the rollout's policy step (egp_policy.hip) and the update's GEMM
// epilogues (egp_gemm.hip) apply the same float32 formulas, so a net evaluates alike in both.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ float egp_act_tanh(float v) { return tanhf(v); }
__device__ __forceinline__ float egp_act_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// d act / d pre-activation from the saved output h = act(pre): the backward pass needs no second save-set
__device__ __forceinline__ float egp_dact_tanh(float h) { return fmaf(-h, h, 1.0f); }        // 1 - h^2
__device__ __forceinline__ float egp_dact_sigmoid(float h) { return h * (1.0f - h); }
