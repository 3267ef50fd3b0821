// Keyed dropout fused with the activation: out = drop(a(y)) and its backward as one streaming pass each (het_amd/layers.py
// KeyedDropout).  The mask is a pure function of (seed, draw, position), recomputed in both passes and never stored.
//
// The rule (all arithmetic uint64, wrapping; sm = sm64 of common.hip.h, the keyed sampler's; i = index in the contiguous tensor):
//   T      = min(llround(p * 65536), 65535)          the effective rate is T / 65536
//   scale  = (float)(65536.0 / (65536 - T))          computed in double, rounded once
//   stream = sm(seed ^ sm(draw))      key(g) = sm(stream + g),  g = (base + i) / 4: one key per 4 consecutive elements
//   field  = (key(g) >> (16 * ((base + i) % 4))) & 0xFFFF        kept(i) = field >= T
//   a(y)   = y (activation 0)  |  y < 0 ? 0 : y (activation 1, relu: a NaN stays a NaN)
//   out[i]    = kept(i) ? a(y[i]) * scale : +0                                    (a select: a dropped NaN or inf is +0)
//   grad_y[i] = kept(i) && (activation == 0 || out[i] > 0) ? grad_out[i] * scale : +0
// bf16 rows are widened (exact), multiplied in fp32 and rounded once, to nearest even, at the store (strow4 / strow1).
//
// One lane takes one group (4 elements: 16 bytes of float, 8 of bf16) per iteration of a grid-stride loop over at most
// kDropMaxBlocks workgroups (8 per CU of a 256-CU part: every wave slot); the last group of a tensor whose length is no multiple of
// 4 is read and written element by element.  Plain vector loads and stores, no LDS, no atomics; every index is 64-bit.
#include <math.h>

#include "common.hip.h"

namespace {

constexpr int kDropMaxBlocks = 2048;  // a lane takes a second group from n > kDropMaxBlocks * kBlock * 4 = 2 097 152 elements on

__device__ __forceinline__ float drop_act(float v, bool relu) { return relu && v < 0.f ? 0.f : v; }

__device__ __forceinline__ float drop_fwd1(float v, uint32_t field, uint32_t T, float scale, bool relu) {
  return field >= T ? drop_act(v, relu) * scale : 0.f;
}
__device__ __forceinline__ float drop_bwd1(float go, float o, uint32_t field, uint32_t T, float scale, bool relu) {
  return field >= T && (!relu || o > 0.f) ? go * scale : 0.f;
}
__device__ __forceinline__ uint32_t drop_field(uint64_t key, int j) { return (uint32_t)(key >> (16 * j)) & 0xffffu; }

// stream_g0 = stream + base / 4: the group of element i is stream_g0 + i / 4
template <typename T, bool RELU>
__global__ __launch_bounds__(kBlock) void HET_keyed_dropout(const T* __restrict__ y, T* __restrict__ out, idx_t n, uint64_t stream_g0,
                                                           uint32_t thr, float scale) {
  const idx_t groups = (n + 3) >> 2;
  const idx_t step = (idx_t)gridDim.x * kBlock;
  for (idx_t g = (idx_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += step) {
    const uint64_t key = sm64(stream_g0 + (uint64_t)g);
    const idx_t i = g << 2;
    if (i + 4 <= n) {
      const float4 v = ldrow4(y + i);
      strow4(out + i, make_float4(drop_fwd1(v.x, drop_field(key, 0), thr, scale, RELU), drop_fwd1(v.y, drop_field(key, 1), thr, scale, RELU),
                                  drop_fwd1(v.z, drop_field(key, 2), thr, scale, RELU), drop_fwd1(v.w, drop_field(key, 3), thr, scale, RELU)));
    } else {
      for (int j = 0; i + j < n; ++j) strow1(out + i + j, drop_fwd1(to_f32(y[i + j]), drop_field(key, j), thr, scale, RELU));
    }
  }
}

// grad_y may be grad_out: a lane reads its group of grad_out before it stores the same group of grad_y, and no other lane touches
// it (so neither pointer is __restrict__).  `out` is read for relu only.
template <typename T, bool RELU>
__global__ __launch_bounds__(kBlock) void HET_keyed_dropout_backward(const T* grad_out, const T* __restrict__ out, T* grad_y, idx_t n,
                                                                    uint64_t stream_g0, uint32_t thr, float scale) {
  const idx_t groups = (n + 3) >> 2;
  const idx_t step = (idx_t)gridDim.x * kBlock;
  for (idx_t g = (idx_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += step) {
    const uint64_t key = sm64(stream_g0 + (uint64_t)g);
    const idx_t i = g << 2;
    if (i + 4 <= n) {
      const float4 go = ldrow4(grad_out + i);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (RELU) o = ldrow4(out + i);
      strow4(grad_y + i, make_float4(drop_bwd1(go.x, o.x, drop_field(key, 0), thr, scale, RELU), drop_bwd1(go.y, o.y, drop_field(key, 1), thr, scale, RELU),
                                     drop_bwd1(go.z, o.z, drop_field(key, 2), thr, scale, RELU), drop_bwd1(go.w, o.w, drop_field(key, 3), thr, scale, RELU)));
    } else {
      for (int j = 0; i + j < n; ++j) {
        const float o = RELU ? to_f32(out[i + j]) : 0.f;
        strow1(grad_y + i + j, drop_bwd1(to_f32(grad_out[i + j]), o, drop_field(key, j), thr, scale, RELU));
      }
    }
  }
}

bool drop_rate(double p, uint32_t& T, float& scale) {
  if (!(p >= 0.0 && p < 1.0)) return false;  // (a NaN fails both comparisons)
  long long t = llround(p * 65536.0);
  if (t > 65535) t = 65535;  // p within 2^-17 of 1: the largest rate that still keeps something
  T = (uint32_t)t;
  scale = (float)(65536.0 / (double)(65536 - t));
  return true;
}

template <typename T>
bool drop_aligned(const T* a, const T* b, const T* c) { return sizeof(T) == 4 ? aligned16(a, b, c) : aligned8(a, b, c); }

template <typename T>
bool drop_overlap(const T* a, const T* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(T);
  return x < y + bytes && y < x + bytes;
}

// the checks the two entries share; -1 = nothing to do (n == 0)
template <typename T>
int drop_check(const char* op, const T* in, const T* saved, const T* result, int64_t n, int64_t base, int activation, double p, uint32_t& thr,
               float& scale) {
  HET_REQUIRE(n >= 0, "%s: n=%lld", op, (long long)n);
  if (n == 0) return -1;
  if (activation != 0 && activation != 1) {
    het_set_error("%s: activation %d (0 = none, 1 = relu)", op, activation);
    return HET_ERR_UNSUPPORTED;
  }
  HET_REQUIRE(in && result, "%s: null pointer", op);
  HET_REQUIRE(drop_aligned(in, saved, result), "%s: misaligned pointer (%d-byte boundaries)", op, (int)(4 * sizeof(T)));
  HET_REQUIRE(base >= 0 && base % 4 == 0, "%s: base=%lld (a multiple of 4, at least 0)", op, (long long)base);
  HET_REQUIRE(drop_rate(p, thr, scale), "%s: p=%g outside [0, 1)", op, p);
  return HET_OK;
}

template <typename T>
int keyed_dropout(const char* op, const T* y, T* out, int64_t n, int64_t base, int activation, double p, int64_t seed, int64_t draw,
                  het_stream stream) {
  uint32_t thr = 0;
  float scale = 1.f;
  const int rc = drop_check(op, y, (const T*)nullptr, (const T*)out, n, base, activation, p, thr, scale);
  if (rc != HET_OK) return rc < 0 ? HET_OK : rc;
  HET_REQUIRE(!drop_overlap(y, (const T*)out, n), "%s: out overlaps y (not an in-place operation)", op);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t stream_g0 = sm64((uint64_t)seed ^ sm64((uint64_t)draw)) + (uint64_t)base / 4;
  const unsigned blocks = grid_for(ceil_div64(n, 4), kDropMaxBlocks);
  HET_KTIME("HET_keyed_dropout", s);
  if (activation)
    hipLaunchKernelGGL((HET_keyed_dropout<T, true>), dim3(blocks), dim3(kBlock), 0, s, y, out, (idx_t)n, stream_g0, thr, scale);
  else
    hipLaunchKernelGGL((HET_keyed_dropout<T, false>), dim3(blocks), dim3(kBlock), 0, s, y, out, (idx_t)n, stream_g0, thr, scale);
  HET_LAUNCH_CHECK("HET_keyed_dropout");
  return HET_OK;
}

template <typename T>
int keyed_dropout_backward(const char* op, const T* grad_out, const T* out, T* grad_y, int64_t n, int64_t base, int activation, double p,
                           int64_t seed, int64_t draw, het_stream stream) {
  uint32_t thr = 0;
  float scale = 1.f;
  const int rc = drop_check(op, grad_out, out, (const T*)grad_y, n, base, activation, p, thr, scale);
  if (rc != HET_OK) return rc < 0 ? HET_OK : rc;
  HET_REQUIRE(!activation || out, "%s: relu needs out (null pointer)", op);
  HET_REQUIRE(!(activation && drop_overlap(out, (const T*)grad_y, n)), "%s: grad_y overlaps out", op);
  HET_REQUIRE(grad_out == grad_y || !drop_overlap(grad_out, (const T*)grad_y, n), "%s: grad_y overlaps grad_out without being it", op);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t stream_g0 = sm64((uint64_t)seed ^ sm64((uint64_t)draw)) + (uint64_t)base / 4;
  const unsigned blocks = grid_for(ceil_div64(n, 4), kDropMaxBlocks);
  HET_KTIME("HET_keyed_dropout_backward", s);
  if (activation)
    hipLaunchKernelGGL((HET_keyed_dropout_backward<T, true>), dim3(blocks), dim3(kBlock), 0, s, grad_out, out, grad_y, (idx_t)n, stream_g0, thr,
                       scale);
  else
    hipLaunchKernelGGL((HET_keyed_dropout_backward<T, false>), dim3(blocks), dim3(kBlock), 0, s, grad_out, (const T*)nullptr, grad_y, (idx_t)n,
                       stream_g0, thr, scale);
  HET_LAUNCH_CHECK("HET_keyed_dropout_backward");
  return HET_OK;
}

}  // namespace

extern "C" int het_keyed_dropout_params(double p, uint32_t* T, float* scale) {
  const char* op = "het_keyed_dropout_params";
  HET_REQUIRE(T && scale, "%s: null pointer", op);
  HET_REQUIRE(drop_rate(p, *T, *scale), "%s: p=%g outside [0, 1)", op, p);
  return HET_OK;
}

extern "C" int het_keyed_dropout(const float* y, float* out, int64_t n, int64_t base, int activation, double p, int64_t seed, int64_t draw,
                                 het_stream stream) {
  return keyed_dropout("het_keyed_dropout", y, out, n, base, activation, p, seed, draw, stream);
}

extern "C" int het_keyed_dropout_bf16(const het_bf16* y, het_bf16* out, int64_t n, int64_t base, int activation, double p, int64_t seed,
                                      int64_t draw, het_stream stream) {
  return keyed_dropout("het_keyed_dropout_bf16", y, out, n, base, activation, p, seed, draw, stream);
}

extern "C" int het_keyed_dropout_backward(const float* grad_out, const float* out, float* grad_y, int64_t n, int64_t base, int activation,
                                          double p, int64_t seed, int64_t draw, het_stream stream) {
  return keyed_dropout_backward("het_keyed_dropout_backward", grad_out, out, grad_y, n, base, activation, p, seed, draw, stream);
}

extern "C" int het_keyed_dropout_backward_bf16(const het_bf16* grad_out, const het_bf16* out, het_bf16* grad_y, int64_t n, int64_t base,
                                               int activation, double p, int64_t seed, int64_t draw, het_stream stream) {
  return keyed_dropout_backward("het_keyed_dropout_backward_bf16", grad_out, out, grad_y, n, base, activation, p, seed, draw, stream);
}
