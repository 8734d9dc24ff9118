// sample_spec.h — the exponential and the integer weight of bridgelang_amd/sampling.py, ONE definition for every kernel
// that has to reproduce them bit for bit: the sampler and scorer (sample.hip) and the beam step (beam.hip).
#pragma once
#include "bl_common.h"

// the widest row those kernels take (bl_sample_f32's limit: its weights live in LDS; sample.hip asserts the figure)
constexpr int kSpecMaxN = 36480;

// e^x for x <= 0: sampling.py::exp_spec operation for operation (contraction off: every multiply and add rounds alone)
__device__ __forceinline__ float exp_spec(float x) {
#pragma clang fp contract(off)
  x = fmaxf(x, -87.0f);
  const float n = rintf(x * 1.44269504f);
  float r = x - n * 0.693359375f;
  r = r - n * -2.12194440e-4f;
  float p = (float)(1.0 / 720);
  p = p * r; p = p + (float)(1.0 / 120);
  p = p * r; p = p + (float)(1.0 / 24);
  p = p * r; p = p + (float)(1.0 / 6);
  p = p * r; p = p + 0.5f;
  p = p * r; p = p + 1.0f;
  p = p * r; p = p + 1.0f;
  const float scale = __builtin_bit_cast(float, (uint32_t)((int)n + 127) << 23);
  return p * scale;
}
__device__ __forceinline__ uint32_t weight_of(float l, float mx, float T) {
#pragma clang fp contract(off)
  const float d = l - mx;
  const float z = d / T;
  const float e = exp_spec(z);
  return (uint32_t)rintf(e * 1073741824.0f);
}
