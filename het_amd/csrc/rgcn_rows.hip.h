// What the RGCN layers share (rgnn_ops.hip: the two-call layer with dense relation weights; rgcn_bdd.hip: the same layer with
// block-diagonal weights): the gather-sum of scaled rows by (relation, node) and the column sums of gradout (the bias gradient).
#pragma once
#include "seg_reduce.hip.h"

namespace {
// column sums of a [rows, 4 * LPR] matrix: per-workgroup partial rows (grid-stride, 16 bytes per lane), finished by HET_colsum_finish
// (T: the element type of `in`, float or het_bf16; the sums are fp32)
template <int LPR, typename T = float>
__global__ __launch_bounds__(256) void HET_colsum_partial(const T* __restrict__ in, int64_t rows, float* __restrict__ part) {
  constexpr int RPI = 256 / LPR;
  __shared__ float4 red[256];
  const int c = threadIdx.x % LPR, r = threadIdx.x / LPR;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = (int64_t)blockIdx.x * RPI + r; i < rows; i += (int64_t)gridDim.x * RPI) {
    const float4 v = ldrow4(in + i * (4 * LPR) + 4 * c);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (r == 0) {
    for (int k = 1; k < RPI; ++k) {
      const float4 v = red[k * LPR + c];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(part + (int64_t)blockIdx.x * (4 * LPR) + 4 * c) = acc;
  }
}
__global__ __launch_bounds__(256) void HET_colsum_finish(const float* __restrict__ part, int P, int X, float* __restrict__ out) {
  __shared__ float red[256];
  const int x = blockIdx.x, t = threadIdx.x;
  float a = 0.f;
  for (int p = t; p < P; p += 256) a += part[(int64_t)p * X + x];
  red[t] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) out[x] = red[0];
}
constexpr int kColsumBlocks = 1024;

template <typename T>
int launch_colsum(const T* in, int64_t rows, int X, float* part, float* out, hipStream_t s) {
  HET_KTIME("HET_colsum", s);
  const int lpr = X / 4;
  const int64_t rpi = 256 / lpr;
  int blocks = (int)(ceil_div64(rows, rpi) < kColsumBlocks ? ceil_div64(rows, rpi) : kColsumBlocks);
  if (blocks < 1) blocks = 1;
  switch (lpr) {
    case 8: hipLaunchKernelGGL((HET_colsum_partial<8, T>), dim3(blocks), dim3(256), 0, s, in, rows, part); break;
    case 16: hipLaunchKernelGGL((HET_colsum_partial<16, T>), dim3(blocks), dim3(256), 0, s, in, rows, part); break;
    case 32: hipLaunchKernelGGL((HET_colsum_partial<32, T>), dim3(blocks), dim3(256), 0, s, in, rows, part); break;
    default: het_set_error("colsum: %d columns unsupported", X); return HET_ERR_UNSUPPORTED;
  }
  HET_LAUNCH_CHECK("HET_colsum_partial");
  hipLaunchKernelGGL(HET_colsum_finish, dim3(X), dim3(256), 0, s, part, blocks, X, out);
  HET_LAUNCH_CHECK("HET_colsum_finish");
  return HET_OK;
}

// ssum[(r,v), :] = SUM over the edges of the segment of norm * in[row, :] -- activation rows of type float or het_bf16, fp32 sums.
// norm_sorted: the norm in the grouping's order (het_grouping_gather_payload1), a coalesced stream instead of a gather per edge.
int rgcn_gather_sum(const het_grouping* g, const float* in, float* out, int X, const float* norm, const float* norm_sorted,
                    hipStream_t s) {
  return launch_segment_sum(g, in, out, X, norm_sorted ? norm_sorted : norm, s, 0, -1, 0, 0, 0, norm_sorted ? 1 : 0);
}
int rgcn_gather_sum(const het_grouping* g, const het_bf16* in, float* out, int X, const float* norm, const float* norm_sorted,
                    hipStream_t s) {
  return launch_segment_sum_bf16(g, in, out, X, norm_sorted ? norm_sorted : norm, s, norm_sorted ? 1 : 0);
}
}  // namespace
