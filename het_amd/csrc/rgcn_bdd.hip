// The RGCN layer with block-diagonal relation weights (DGL's RelGraphConv(regularizer="bdd")): include/het_amd.h,
// het_rgcn_bdd_layer_forward / _backward.  weight [R, B, si, so], si = K / B, so = D / B:
//   out[v, b*so + j] = bias[b*so + j] + SUM_r SUM_{e: rel r, dst v} norm_e * SUM_i x[src_e, b*si + i] * weight[r, b, i, j]
// The dataflow is the two-call layer's (rgnn_ops.hip): the gather-sum by (relation, node) stays (rgcn_rows.hip.h),
// the two dense node passes and the weight gradient are the kernels of this file.  A relation costs K*D/B floats, so hundreds of
// relations stay cache resident and nothing here is sized by R x N: a node finds its (relation, node) rows through a per-node list
// (het_grouping_node_rows) built from the grouping's own segment list by a stable sort by node -- a node's entries are in ascending
// relation order, which fixes the order of every sum below.  Every output is stored once by plain stores; sums that meet in one
// output are added in a fixed order (rows of a node in list order, chunk partials in chunk order).
#include <hipcub/hipcub.hpp>

#include "device_scratch.hip.h"
#include "rgcn_rows.hip.h"

namespace {

constexpr int kBddBlock = 256;               // threads of every workgroup of this file
constexpr int kBddChunkRows = 1024;          // (relation, node) rows of one weight-gradient work item
constexpr int kBddLdsWeightBytes = 64 * 1024;  // all R relations' blocks are staged in LDS up to this many bytes (two workgroups per CU)
constexpr int kBddMinSide = 4, kBddMaxSide = 32;  // si and so: powers of two in this range

// ---- the per-node row list ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBddBlock) void HET_bdd_iota(int32_t* __restrict__ v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBddBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBddBlock) v[i] = (int32_t)i;
}

// node_ptr[n] = first position of the sorted keys that is >= n (n = 0 .. N: node_ptr[N] = S);  ent_rel[e] = relation of segment ent_row[e]
__global__ __launch_bounds__(kBddBlock) void HET_bdd_node_rows_finish(const int32_t* __restrict__ keys_sorted, int64_t S,
                                                                       const int32_t* __restrict__ seg_rel_ptr, int R,
                                                                       const int32_t* __restrict__ ent_row, int64_t N,
                                                                       int32_t* __restrict__ node_ptr, int32_t* __restrict__ ent_rel) {
  const int64_t stride = (int64_t)gridDim.x * kBddBlock, t0 = (int64_t)blockIdx.x * kBddBlock + threadIdx.x;
  for (int64_t n = t0; n <= N; n += stride) {
    int64_t lo = 0, hi = S;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys_sorted[mid] < n) lo = mid + 1; else hi = mid;
    }
    node_ptr[n] = (int32_t)lo;
  }
  for (int64_t e = t0; e < S; e += stride) {
    const int32_t row = ent_row[e];
    int lo = 0, hi = R;  // the relation r with seg_rel_ptr[r] <= row < seg_rel_ptr[r + 1] (empty relations allowed)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (seg_rel_ptr[mid] <= row) lo = mid; else hi = mid;
    }
    ent_rel[e] = lo;
  }
}

// ---- the node-major pass ---------------------------------------------------------------------------------------------------
// out[n, :] = bias + SUM over the entries (row, r) of node n, in list order, of rows[row, :] . blockdiag(w[r]);   w [R][B][SI][so].
// D / 4 lanes per node, a lane owns 4 consecutive output columns (they lie in one block: so >= 4) and reads its block's SI input
// floats (the lanes of a block read the same 16-byte pieces: one request) and SI 16-byte pieces of the block per entry.
// LDSW: the blocks of all relations are staged in LDS once per workgroup; otherwise they are read through the caches.
struct BddNodeArgs {
  const float* rows;        // [*, K] the (relation, node) sums
  const int32_t* node_ptr;  // [N + 1]
  const int32_t* ent_row;   // [S]
  const int32_t* ent_rel;   // [S]
  const float* w;           // [R][B][SI][so]
  const float* bias;        // [D] or NULL
  float* out;               // [N, D]
  int64_t N;
  int R, K, D, so;
};

template <int SI, bool LDSW>
__global__ __launch_bounds__(kBddBlock) void HET_rgcn_bdd_node_pass(BddNodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float bdd_smem[];
  const int tid = threadIdx.x;
  const int wrel = SI * a.D;  // floats of one relation
  if (LDSW) {
    const float4* src = reinterpret_cast<const float4*>(a.w);
    float4* dst = reinterpret_cast<float4*>(bdd_smem);
    const int total4 = a.R * (wrel / 4);
    for (int e = tid; e < total4; e += kBddBlock) dst[e] = src[e];
    __syncthreads();
  }
  const int lpn = a.D >> 2, npb = kBddBlock / lpn;
  const int l = tid % lpn, sub = tid / lpn;
  const int d0 = 4 * l, b = d0 / a.so, j0 = d0 - b * a.so;
  const int woff = b * SI * a.so + j0;  // this lane's first float inside a relation's blocks
  const float4 bias4 = a.bias ? ld4(a.bias + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t tiles = (a.N + npb - 1) / npb;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t n = t * npb + sub;
    if (n >= a.N) continue;
    int e = a.node_ptr[n];
    const int end = a.node_ptr[n + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int row = 0, rel = 0;
    if (e < end) { row = a.ent_row[e]; rel = a.ent_rel[e]; }
    while (e < end) {
      int nrow = 0, nrel = 0;
      if (e + 1 < end) { nrow = a.ent_row[e + 1]; nrel = a.ent_rel[e + 1]; }  // (in flight during this entry's products)
      const float* xp = a.rows + (int64_t)row * a.K + b * SI;
      float x[SI];
#pragma unroll
      for (int q = 0; q < SI / 4; ++q) {
        const float4 v = ld4(xp + 4 * q);
        x[4 * q + 0] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int i = 0; i < SI; ++i) {
        float4 w4;
        if (LDSW) w4 = *reinterpret_cast<const float4*>(&bdd_smem[rel * wrel + woff + i * a.so]);
        else w4 = ld4(a.w + (int64_t)rel * wrel + woff + i * a.so);
        acc.x = fmaf(x[i], w4.x, acc.x); acc.y = fmaf(x[i], w4.y, acc.y);
        acc.z = fmaf(x[i], w4.z, acc.z); acc.w = fmaf(x[i], w4.w, acc.w);
      }
      row = nrow; rel = nrel; ++e;
    }
    acc.x += bias4.x; acc.y += bias4.y; acc.z += bias4.z; acc.w += bias4.w;
    st4(a.out + n * a.D + d0, acc);  // (a node without entries: the bias, or zeros)
  }
}

bool bdd_weights_in_lds(int64_t R, int64_t K, int64_t D, int64_t B) {
  const int64_t bytes = R * (K * D / B) * (int64_t)sizeof(float);
  return bytes <= kBddLdsWeightBytes && (size_t)bytes <= het_lds_budget();
}

template <int SI>
int launch_bdd_node_pass(const BddNodeArgs& a, bool ldsw, hipStream_t s) {
  HET_KTIME("HET_rgcn_bdd_node_pass", s);
  const int npb = kBddBlock / (a.D / 4);
  const int64_t tiles = (a.N + npb - 1) / npb, cus = het_num_cus();
  int64_t gx = tiles < (ldsw ? 2 : 8) * cus ? tiles : (ldsw ? 2 : 8) * cus;
  if (gx < 1) gx = 1;
  if (ldsw) {
    const size_t lds = sizeof(float) * (size_t)a.R * SI * a.D;
    HET_HIP(hipFuncSetAttribute((const void*)HET_rgcn_bdd_node_pass<SI, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((HET_rgcn_bdd_node_pass<SI, true>), dim3((unsigned)gx), dim3(kBddBlock), lds, s, a);
  } else {
    hipLaunchKernelGGL((HET_rgcn_bdd_node_pass<SI, false>), dim3((unsigned)gx), dim3(kBddBlock), 0, s, a);
  }
  HET_LAUNCH_CHECK("HET_rgcn_bdd_node_pass");
  return HET_OK;
}

// rows [*, KS] -> out [N, XO] through w [R][B][KS/B][XO/B]
int bdd_node_pass(const float* rows, const int32_t* node_ptr, const int32_t* ent_row, const int32_t* ent_rel, const float* w,
                  const float* bias, float* out, int64_t N, int64_t R, int64_t KS, int64_t XO, int64_t B, hipStream_t s) {
  BddNodeArgs a{rows, node_ptr, ent_row, ent_rel, w, bias, out, N, (int)R, (int)KS, (int)XO, (int)(XO / B)};
  const bool ldsw = bdd_weights_in_lds(R, KS, XO, B);
  switch (KS / B) {
    case 4: return launch_bdd_node_pass<4>(a, ldsw, s);
    case 8: return launch_bdd_node_pass<8>(a, ldsw, s);
    case 16: return launch_bdd_node_pass<16>(a, ldsw, s);
    default: return launch_bdd_node_pass<32>(a, ldsw, s);
  }
}

// ---- the block weight gradient ---------------------------------------------------------------------------------------------
// grad_w[r, b, i, j] = SUM over the rows s of relation r (contiguous: seg_rel_ptr) of ssum[s, b*SI + i] * gradout[seg_key[s], b*so + j].
// Work item = (relation, chunk of kBddChunkRows rows).  Relation r owns the partial slots [slot(r), slot(r + 1)),
// slot(r) = seg_rel_ptr[r] / chunk + r: strictly increasing, at least ceil(rows / chunk) slots each, S / chunk + R in all, and
// computable from seg_rel_ptr alone -- no prefix sum, no read-back.  A slot past the relation's last chunk is neither written nor read.
__device__ __forceinline__ int bdd_slot(const int32_t* __restrict__ seg_rel_ptr, int r) { return seg_rel_ptr[r] / kBddChunkRows + r; }

template <int SI>
__global__ __launch_bounds__(kBddBlock) void HET_rgcn_bdd_dw(const float* __restrict__ ssum, int K, const float* __restrict__ gradout,
                                                              int D, int so, const int32_t* __restrict__ seg_key,
                                                              const int32_t* __restrict__ seg_rel_ptr, int R,
                                                              float* __restrict__ part) {
  __shared__ float red[kBddBlock * SI];  // [256 / D groups][SI * D]
  const int w = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = R;  // the relation whose slots hold w
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (bdd_slot(seg_rel_ptr, mid) <= w) lo = mid; else hi = mid;
  }
  const int r = lo, c = w - bdd_slot(seg_rel_ptr, r);
  const int p0 = seg_rel_ptr[r], n = seg_rel_ptr[r + 1] - p0;
  if ((int64_t)c * kBddChunkRows >= n) return;  // (uniform for the workgroup)
  const int begin = p0 + c * kBddChunkRows;
  const int end = (n - c * kBddChunkRows > kBddChunkRows) ? begin + kBddChunkRows : p0 + n;
  const int d = tid % D, grp = tid / D, G = kBddBlock / D;
  const int b = d / so, j = d - b * so;
  const int W = SI * D;
  float acc[SI];
#pragma unroll
  for (int i = 0; i < SI; ++i) acc[i] = 0.f;
  // (several rows in flight per lane; the order of the adds is the loop's)
  auto add_row = [&](int s) {
    const float g = gradout[(int64_t)seg_key[s] * D + d];
    const float* xp = ssum + (int64_t)s * K + b * SI;
#pragma unroll
    for (int q = 0; q < SI / 4; ++q) {
      const float4 v = ld4(xp + 4 * q);
      acc[4 * q + 0] = fmaf(v.x, g, acc[4 * q + 0]); acc[4 * q + 1] = fmaf(v.y, g, acc[4 * q + 1]);
      acc[4 * q + 2] = fmaf(v.z, g, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(v.w, g, acc[4 * q + 3]);
    }
  };
  if (SI <= 8) {
#pragma unroll 8
    for (int s = begin + grp; s < end; s += G) add_row(s);
  } else {
#pragma unroll 4
    for (int s = begin + grp; s < end; s += G) add_row(s);
  }
#pragma unroll
  for (int i = 0; i < SI; ++i) red[grp * W + b * SI * so + i * so + j] = acc[i];
  __syncthreads();
  for (int e = tid; e < W; e += kBddBlock) {
    float v = red[e];
    for (int k = 1; k < G; ++k) v += red[k * W + e];
    part[(int64_t)w * W + e] = v;
  }
}

// grad_w[r] = the chunk partials of relation r added in chunk order (zeros for a relation without rows)
__global__ __launch_bounds__(kBddBlock) void HET_rgcn_bdd_dw_finish(const float* __restrict__ part, const int32_t* __restrict__ seg_rel_ptr,
                                                                     int W, float* __restrict__ grad_w) {
  const int r = blockIdx.x;
  const int n = seg_rel_ptr[r + 1] - seg_rel_ptr[r];
  const int chunks = (n + kBddChunkRows - 1) / kBddChunkRows;
  const float* p = part + (int64_t)bdd_slot(seg_rel_ptr, r) * W;
  for (int e = threadIdx.x; e < W; e += kBddBlock) {
    float v = 0.f;
    for (int c = 0; c < chunks; ++c) v += p[(int64_t)c * W + e];
    grad_w[(int64_t)r * W + e] = v;
  }
}

int64_t bdd_dw_slots(int64_t n_rows, int64_t R) { return n_rows / kBddChunkRows + R; }

int launch_bdd_dw(const het_grouping* gd, const float* ssum, const float* gradout, float* part, float* grad_w, int64_t R, int64_t K,
                  int64_t D, int64_t B, hipStream_t s) {
  const int si = (int)(K / B), so = (int)(D / B);
  const unsigned slots = (unsigned)bdd_dw_slots(gd->S, R);
  if (gd->S > 0) {
    HET_KTIME("HET_rgcn_bdd_dw", s);
    switch (si) {
      case 4: hipLaunchKernelGGL(HET_rgcn_bdd_dw<4>, dim3(slots), dim3(kBddBlock), 0, s, ssum, (int)K, gradout, (int)D, so, gd->seg_key, gd->seg_rel_ptr, (int)R, part); break;
      case 8: hipLaunchKernelGGL(HET_rgcn_bdd_dw<8>, dim3(slots), dim3(kBddBlock), 0, s, ssum, (int)K, gradout, (int)D, so, gd->seg_key, gd->seg_rel_ptr, (int)R, part); break;
      case 16: hipLaunchKernelGGL(HET_rgcn_bdd_dw<16>, dim3(slots), dim3(kBddBlock), 0, s, ssum, (int)K, gradout, (int)D, so, gd->seg_key, gd->seg_rel_ptr, (int)R, part); break;
      default: hipLaunchKernelGGL(HET_rgcn_bdd_dw<32>, dim3(slots), dim3(kBddBlock), 0, s, ssum, (int)K, gradout, (int)D, so, gd->seg_key, gd->seg_rel_ptr, (int)R, part); break;
    }
    HET_LAUNCH_CHECK("HET_rgcn_bdd_dw");
  }
  HET_KTIME("HET_rgcn_bdd_dw_finish", s);
  hipLaunchKernelGGL(HET_rgcn_bdd_dw_finish, dim3((unsigned)R), dim3(kBddBlock), 0, s, part, gd->seg_rel_ptr, si * (int)D, grad_w);
  HET_LAUNCH_CHECK("HET_rgcn_bdd_dw_finish");
  return HET_OK;
}

bool bdd_side_ok(int64_t v) { return v >= kBddMinSide && v <= kBddMaxSide && is_pow2(v); }
bool bdd_width_ok(int64_t X) { return (X == 32 || X == 64 || X == 128) && segment_sum_supported((int)X); }
bool bdd_shape_ok(int64_t R, int64_t K, int64_t D, int64_t B) {
  return R >= 1 && R < (1ll << 20) && B >= 1 && bdd_width_ok(K) && bdd_width_ok(D) && K % B == 0 && D % B == 0 && bdd_side_ok(K / B) &&
         bdd_side_ok(D / B);
}

// HET_ERR_UNSUPPORTED with the entry's name for a shape outside het_rgcn_bdd_layer_ok (sizes that make no sense at all: HET_ERR_INVALID_ARG)
int bdd_check_shape(const char* op, int64_t R, int64_t K, int64_t D, int64_t B) {
  HET_REQUIRE(R >= 1 && K >= 1 && D >= 1 && B >= 1, "%s: bad sizes: R=%lld K=%lld D=%lld B=%lld", op, (long long)R, (long long)K,
              (long long)D, (long long)B);
  if (!bdd_shape_ok(R, K, D, B)) {
    het_set_error("%s: unsupported shape R=%lld K=%lld D=%lld B=%lld (het_rgcn_bdd_layer_ok: K, D in {32, 64, 128}, K/B and D/B in {4, 8, 16, 32})",
                  op, (long long)R, (long long)K, (long long)D, (long long)B);
    return HET_ERR_UNSUPPORTED;
  }
  return HET_OK;
}

}  // namespace

extern "C" int het_rgcn_bdd_params(int64_t* out) {
  HET_REQUIRE(out, "het_rgcn_bdd_params: null pointer");
  out[0] = kBddChunkRows;
  out[1] = kBddLdsWeightBytes;
  out[2] = kBddBlock;
  out[3] = kBddMinSide;
  out[4] = kBddMaxSide;
  out[5] = kColsumBlocks;
  return HET_OK;
}

extern "C" int het_rgcn_bdd_layer_ok(int64_t num_rels, int64_t K, int64_t D, int64_t B) { return bdd_shape_ok(num_rels, K, D, B) ? 1 : 0; }

extern "C" int64_t het_rgcn_bdd_layer_backward_workspace(int64_t n_src_rows, int64_t n_dst_rows, int64_t num_rels, int64_t K, int64_t D,
                                                         int64_t B) {
  if (n_src_rows < 0 || n_dst_rows < 0 || !bdd_shape_ok(num_rels, K, D, B)) {
    het_set_error("het_rgcn_bdd_layer_backward_workspace: negative row count or unsupported shape R=%lld K=%lld D=%lld B=%lld",
                  (long long)num_rels, (long long)K, (long long)D, (long long)B);
    return -1;
  }
  return (int64_t)sizeof(float) * ((n_src_rows > 0 ? n_src_rows : 1) * D + (int64_t)kColsumBlocks * D +
                                   bdd_dw_slots(n_dst_rows, num_rels) * (K / B) * D);
}

extern "C" int het_grouping_node_rows(const het_grouping* g, int64_t num_keys, int32_t* node_ptr, int32_t* ent_row, int32_t* ent_rel,
                                      het_stream stream) {
  const char* op = "het_grouping_node_rows";
  HET_REQUIRE(num_keys >= 0 && num_keys < (1ll << 31), "%s: num_keys=%lld", op, (long long)num_keys);
  HET_REQUIRE(g && node_ptr, "%s: null grouping or node_ptr", op);
  HET_REQUIRE(g->R > 0 && num_keys >= g->key_bound, "%s: needs a grouping by (relation, key) and num_keys >= its key bound", op);
  HET_REQUIRE(g->S == 0 || (ent_row && ent_rel), "%s: null entry list", op);
  hipStream_t s = (hipStream_t)stream;
  const int64_t S = g->S;
  Scratch tmp(s);
  int32_t* keys_sorted = nullptr;
  if (S > 0) {
    int32_t* iota = nullptr;
    void* t0 = nullptr;
    size_t tb = 0;
    const int bits = bits_for(g->key_bound);
    HET_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, g->seg_key, keys_sorted, iota, ent_row, (int)S, 0, bits, s));
    HET_HIP(tmp.alloc((void**)&keys_sorted, sizeof(int32_t) * S));
    HET_HIP(tmp.alloc((void**)&iota, sizeof(int32_t) * S));
    HET_HIP(tmp.alloc(&t0, tb));
    hipLaunchKernelGGL(HET_bdd_iota, dim3(grid_for(S)), dim3(kBddBlock), 0, s, iota, S);
    HET_LAUNCH_CHECK("HET_bdd_iota");
    // (a radix sort is stable: the segments of a node keep their (relation, key) order, i.e. ascending relations)
    HET_HIP(hipcub::DeviceRadixSort::SortPairs(t0, tb, g->seg_key, keys_sorted, iota, ent_row, (int)S, 0, bits, s));
  }
  const int64_t work = num_keys + 1 > S ? num_keys + 1 : S;
  hipLaunchKernelGGL(HET_bdd_node_rows_finish, dim3(grid_for(work)), dim3(kBddBlock), 0, s, keys_sorted, S, g->seg_rel_ptr, g->R, ent_row,
                     num_keys, node_ptr, ent_rel);
  HET_LAUNCH_CHECK("HET_bdd_node_rows_finish");
  return HET_OK;
}

extern "C" int het_rgcn_bdd_layer_forward(const het_grouping* by_rel_dst, int64_t num_rels, int64_t num_nodes, const float* x,
                                          const float* weights, const float* norm, const float* norm_sorted, const float* bias,
                                          const int32_t* node_ptr, const int32_t* ent_row, const int32_t* ent_rel, float* ssum,
                                          float* ret, int64_t K, int64_t D, int64_t B, het_stream stream) {
  const char* op = "het_rgcn_bdd_layer_forward";
  if (int rc = bdd_check_shape(op, num_rels, K, D, B)) return rc;
  HET_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "%s: bad node count %lld", op, (long long)num_nodes);
  HET_REQUIRE(aligned16(x, weights, bias, ssum, ret), "%s: x, weights, bias, ssum and ret must be 16-byte aligned", op);
  const het_grouping* g = by_rel_dst;
  HET_REQUIRE(g && g->R == (int)num_rels && g->p0 && g->p1 && num_nodes >= g->key_bound,
              "%s: needs the grouping by (relation, destination) with payloads (source row, edge id) of a graph of at most num_nodes nodes", op);
  if (num_nodes == 0) return HET_OK;
  HET_REQUIRE(x && weights && (norm || norm_sorted) && node_ptr && ret && (g->S == 0 || (ent_row && ent_rel && ssum)), "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  if (g->E > 0)
    if (int rc = rgcn_gather_sum(g, x, ssum, (int)K, norm, norm_sorted, s)) return rc;
  return bdd_node_pass(ssum, node_ptr, ent_row, ent_rel, weights, bias, ret, num_nodes, num_rels, K, D, B, s);
}

extern "C" int het_rgcn_bdd_layer_backward(const het_grouping* by_rel_src, const het_grouping* by_rel_dst, int64_t num_rels,
                                           int64_t num_src_nodes, int64_t num_dst_nodes, const float* ssum, const float* weights_t,
                                           const float* norm, const float* norm_sorted, const float* gradout, const int32_t* node_ptr,
                                           const int32_t* ent_row, const int32_t* ent_rel, float* grad_x, float* grad_w, float* grad_bias,
                                           int64_t K, int64_t D, int64_t B, void* workspace, int64_t workspace_bytes, het_stream stream) {
  const char* op = "het_rgcn_bdd_layer_backward";
  if (int rc = bdd_check_shape(op, num_rels, K, D, B)) return rc;
  HET_REQUIRE(num_src_nodes >= 0 && num_src_nodes < (1ll << 31) && num_dst_nodes >= 0 && num_dst_nodes < (1ll << 31),
              "%s: bad node counts %lld, %lld", op, (long long)num_src_nodes, (long long)num_dst_nodes);
  HET_REQUIRE(aligned16(ssum, weights_t, gradout, grad_x, grad_w, workspace), "%s: ssum, weights_t, gradout, grad_x, grad_w and the workspace must be 16-byte aligned", op);
  HET_REQUIRE(workspace && workspace_bytes >= het_rgcn_bdd_layer_backward_workspace(0, 0, num_rels, K, D, B),
              "%s: workspace too small (het_rgcn_bdd_layer_backward_workspace)", op);
  const het_grouping *gs = by_rel_src, *gd = by_rel_dst;
  HET_REQUIRE(gs && gd && gs->R == (int)num_rels && gd->R == (int)num_rels && gs->E == gd->E && gs->p0 && gs->p1 &&
                  num_dst_nodes >= gd->key_bound && num_src_nodes >= gs->key_bound,
              "%s: needs the groupings by (relation, source) [payloads: destination row, edge id] and by (relation, destination)", op);
  HET_REQUIRE(workspace_bytes >= het_rgcn_bdd_layer_backward_workspace(gs->S, gd->S, num_rels, K, D, B),
              "%s: workspace too small (het_rgcn_bdd_layer_backward_workspace)", op);
  HET_REQUIRE(grad_w && (gd->S == 0 || (ssum && gradout)) && (!grad_bias || gradout || num_dst_nodes == 0) &&
                  (!grad_x || num_src_nodes == 0 || (weights_t && (norm || norm_sorted) && node_ptr && gradout && (gs->S == 0 || (ent_row && ent_rel)))),
              "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  float* gsum = static_cast<float*>(workspace);
  float* cpart = gsum + (gs->S > 0 ? gs->S : 1) * D;
  float* wpart = cpart + (int64_t)kColsumBlocks * D;
  auto weight_gradients = [&](hipStream_t st) -> int {
    if (int rc = launch_bdd_dw(gd, ssum, gradout, wpart, grad_w, num_rels, K, D, B, st)) return rc;
    if (grad_bias)
      if (int rc = launch_colsum(gradout, num_dst_nodes, (int)D, cpart, grad_bias, st)) return rc;
    return HET_OK;
  };
  // grad_x NULL: the layer input needs no gradient -- the source-side gather and the node pass are skipped
  if (!grad_x || num_src_nodes == 0) return weight_gradients(s);
  if (gs->E > 0)
    if (int rc = rgcn_gather_sum(gs, gradout, gsum, (int)D, norm, norm_sorted, s)) return rc;
  HetFork fk(s);
  if (int rc = weight_gradients(fk.side)) return rc;
  // grad_x[u, :] = SUM over the entries of u of gsum[row, :] . blockdiag(weight[r])^T: the forward's pass with D and K exchanged
  if (int rc = bdd_node_pass(gsum, node_ptr, ent_row, ent_rel, weights_t, nullptr, grad_x, num_src_nodes, num_rels, D, K, B, s)) return rc;
  HET_HIP(fk.join());
  return HET_OK;
}
