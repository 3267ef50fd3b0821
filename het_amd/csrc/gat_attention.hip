// The attention weights of the compact RGAT layer as an output (het_rgat_attention_compact):
//   attn[eid, h] = exp(leaky(el_c[srow_e, h] + er_c[drow_e, h]) - lse[dst_e, h]),  lse[v, h] = log SUM_{e into v} exp(leaky(..)).
//
// The aggregation kernels (gat_compact.hip) form these weights inside their gather walk and never store them.  This pass reads
// the ids and the two small tables el_c [S_row,H] / er_c [S_col,H] only -- never a feat_c row -- in two phases:
//   1  lse [N,H]: the work items of the grouping by destination (payload0 = feat row, payload1 = er row), a group of 8 edge slots
//      per item, every lane a running {max, sum} per head over its edges (any score is safe), one store per destination.  A
//      destination of more than HET_ITEM_MAX in-edges owns several items: each parks {max[H], sum[H]} in the workspace and a wave
//      per such destination combines the records in a fixed order.  No float atomics: the same bits run after run.
//   2  attn [E,H]: all heads of an edge are one 4*H-byte row (a lane per edge up to 4 heads, two lanes at 8 heads, 16-byte
//      accesses from 4 heads on).  Two orders (HET_RGAT_ATTN_ORDER; DESIGN.md 4.2 has the measurement):
//        positions     coalesced col / srow / drow / eids, three 4*H-byte gathers (el_c, er_c, lse), rows stored at eids[p]
//        destinations  the grouping's sorted ranks: coalesced key / srow / drow / perm, er_c and lse rows shared by neighbouring
//                      lanes, one gather (el_c), an 8-byte eids gather and a scattered store
// Everything is fp32 whatever the layer's activation type: el_c and er_c are fp32 in the bf16 layer too.
#include <math.h>
#include <stdlib.h>

#include "grouping.hip.h"

namespace {

__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.f ? z : slope * z; }

// HL consecutive floats (1, 2 or 4) with one access
template <int HL>
__device__ __forceinline__ void ld_heads(const float* __restrict__ p, float (&v)[HL]) {
  if constexpr (HL == 1) {
    v[0] = p[0];
  } else if constexpr (HL == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
    const float4 t = ld4(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
}
template <int HL>
__device__ __forceinline__ void st_heads(float* __restrict__ p, const float (&v)[HL]) {
  if constexpr (HL == 1) {
    p[0] = v[0];
  } else if constexpr (HL == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
    st4(p, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// {m, s} <- {m, s} (+) {mo, so}: sums of exponentials relative to a maximum; a side that saw no edge has m == -inf, s == 0
__device__ __forceinline__ void lse_merge(float& m, float& s, float mo, float so) {
  const float mn = fmaxf(m, mo);
  const float a = m == -INFINITY ? 0.f : s * expf(m - mn);
  const float b = mo == -INFINITY ? 0.f : so * expf(mo - mn);
  s = a + b;
  m = mn;
}

__global__ __launch_bounds__(kBlock) void HET_rgat_attn_fill(float* __restrict__ p, int64_t n, float v) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) p[i] = v;
}

// Phase 1.  H heads = LPE lanes of HL heads each; a group of G = 8 * LPE lanes per work item, 64 / G items per wave.
template <int H>
__global__ __launch_bounds__(kBlock) void HET_rgat_attn_lse(Items it, const int32_t* __restrict__ p_srow,
                                                             const int32_t* __restrict__ p_drow, const float* __restrict__ el,
                                                             const float* __restrict__ er, float slope, float* __restrict__ lse,
                                                             float* __restrict__ part) {
  constexpr int HL = H < 4 ? H : 4, LPE = H / HL, SLOTS = 8, G = SLOTS * LPE, IPW = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = sub / LPE, hoff = (sub % LPE) * HL;
  const int64_t item = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * IPW + lane / G;
  if (item >= it.n) return;  // (the whole group leaves: the shuffles below stay inside a group)
  const int seg = it.seg[item], b = it.begin[item], e = it.end[item];
  float m[HL], s[HL];
#pragma unroll
  for (int k = 0; k < HL; ++k) { m[k] = -INFINITY; s[k] = 0.f; }
  for (int j = b + slot; j < e; j += SLOTS) {
    const int64_t sr = p_srow[j], dr = p_drow[j];
    float zl[HL], zr[HL];
    ld_heads<HL>(el + sr * H + hoff, zl);
    ld_heads<HL>(er + dr * H + hoff, zr);
#pragma unroll
    for (int k = 0; k < HL; ++k) lse_merge(m[k], s[k], lrelu(zl[k] + zr[k], slope), 1.f);
  }
#pragma unroll
  for (int off = LPE; off < G; off <<= 1) {
#pragma unroll
    for (int k = 0; k < HL; ++k) {
      const float mo = __shfl_xor(m[k], off), so = __shfl_xor(s[k], off);
      lse_merge(m[k], s[k], mo, so);
    }
  }
  if (slot != 0) return;
  if (b == it.seg_ptr[seg] && e == it.seg_ptr[seg + 1]) {  // a whole destination (it has an edge: m is finite)
    float L[HL];
#pragma unroll
    for (int k = 0; k < HL; ++k) L[k] = m[k] + logf(s[k]);
    st_heads<HL>(lse + (int64_t)it.seg_key[seg] * H + hoff, L);
  } else {  // a piece of a split destination: parked for HET_rgat_attn_lse_finish
    float* pp = part + item * (2 * H);
    st_heads<HL>(pp + hoff, m);
    st_heads<HL>(pp + H + hoff, s);
  }
}

// One wave per split destination: the {max[H], sum[H]} records of its items (consecutive: HET_grouping_items), lane i takes the
// records i, i + 64, ... in order, then the lanes meet in a butterfly -- a fixed order, whatever order split_seg lists the segments in.
template <int H>
__global__ __launch_bounds__(kBlock) void HET_rgat_attn_lse_finish(const int32_t* __restrict__ split_seg, int64_t num_split, Items it,
                                                                    const float* __restrict__ part, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (k >= num_split) return;
  const int seg = split_seg[k];
  int64_t lo = 0, hi = it.n;  // first work item of the segment (items are in segment order)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (it.seg[mid] < seg) lo = mid + 1; else hi = mid;
  }
  const int64_t n_items = (it.seg_ptr[seg + 1] - it.seg_ptr[seg] + HET_ITEM_MAX - 1) / HET_ITEM_MAX;
  float m[H], s[H];
#pragma unroll
  for (int h = 0; h < H; ++h) { m[h] = -INFINITY; s[h] = 0.f; }
  for (int64_t i = lane; i < n_items; i += 64) {
    const float* pp = part + (lo + i) * (2 * H);
#pragma unroll
    for (int h = 0; h < H; ++h) lse_merge(m[h], s[h], pp[h], pp[H + h]);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float mo = __shfl_xor(m[h], off), so = __shfl_xor(s[h], off);
      lse_merge(m[h], s[h], mo, so);
    }
  }
  if (lane < H) {
    float L = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h) if (h == lane) L = m[h] + logf(s[h]);
    lse[(int64_t)it.seg_key[seg] * H + lane] = L;
  }
}

template <int HL>
__device__ __forceinline__ void attn_row(const float* __restrict__ el, const float* __restrict__ er, const float* __restrict__ lse,
                                         float slope, float* __restrict__ out) {
  float zl[HL], zr[HL], L[HL], a[HL];
  ld_heads<HL>(el, zl);
  ld_heads<HL>(er, zr);
  ld_heads<HL>(lse, L);
#pragma unroll
  for (int k = 0; k < HL; ++k) a[k] = expf(lrelu(zl[k] + zr[k], slope) - L[k]);
  st_heads<HL>(out, a);
}

// Phase 2 in edge-position order.  eids NULL: the row of position p is p.
template <int H>
__global__ __launch_bounds__(kBlock) void HET_rgat_attn_rows(const idx_t* __restrict__ col, const idx_t* __restrict__ srow,
                                                              const idx_t* __restrict__ drow, const idx_t* __restrict__ eids,
                                                              int64_t E, const float* __restrict__ el, const float* __restrict__ er,
                                                              const float* __restrict__ lse, float slope, float* __restrict__ attn) {
  constexpr int HL = H < 4 ? H : 4, LPE = H / HL;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t p = t / LPE;
  if (p >= E) return;
  const int hoff = (int)(t % LPE) * HL;
  const idx_t v = col[p], sr = srow[p], dr = drow[p], row = eids ? eids[p] : p;
  attn_row<HL>(el + sr * H + hoff, er + dr * H + hoff, lse + v * H + hoff, slope, attn + row * H + hoff);
}

// Phase 2 in the order of the grouping by destination (sorted rank j: destination key[j], rows p0[j] / p1[j], position perm[j]).
template <int H>
__global__ __launch_bounds__(kBlock) void HET_rgat_attn_rows_by_dst(const int32_t* __restrict__ key, const int32_t* __restrict__ p_srow,
                                                                     const int32_t* __restrict__ p_drow, const int32_t* __restrict__ perm,
                                                                     const idx_t* __restrict__ eids, int64_t E,
                                                                     const float* __restrict__ el, const float* __restrict__ er,
                                                                     const float* __restrict__ lse, float slope,
                                                                     float* __restrict__ attn) {
  constexpr int HL = H < 4 ? H : 4, LPE = H / HL;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t j = t / LPE;
  if (j >= E) return;
  const int hoff = (int)(t % LPE) * HL;
  const int64_t v = key[j], sr = p_srow[j], dr = p_drow[j], p = perm[j];
  const int64_t row = eids ? eids[p] : p;
  attn_row<HL>(el + sr * H + hoff, er + dr * H + hoff, lse + v * H + hoff, slope, attn + row * H + hoff);
}

}  // namespace

#define HET_DISPATCH_HEADS(HV, CALL)                \
  switch (HV) {                                     \
    case 1: { constexpr int H = 1; CALL; break; }   \
    case 2: { constexpr int H = 2; CALL; break; }   \
    case 4: { constexpr int H = 4; CALL; break; }   \
    default: { constexpr int H = 8; CALL; break; }  \
  }

static bool attn_heads_ok(int64_t H) { return H == 1 || H == 2 || H == 4 || H == 8; }
static int64_t round16(int64_t b) { return (b + 15) / 16 * 16; }

// phase 2 walks the destination grouping instead of the edge positions (A/B: exp/rgat_attention_ab.py); read at every call, so a
// process can run both orders (tests/test_gpu_rgat_attention.py does)
static bool attn_by_dst() {
  const char* e = getenv("HET_RGAT_ATTN_ORDER");
  return e && e[0] == 'd';
}

extern "C" int64_t het_rgat_attention_compact_workspace(const het_grouping* by_dst, int64_t H, int64_t num_nodes, int with_lse_out) {
  if (!by_dst || !attn_heads_ok(H) || num_nodes < 0) return -1;
  const int64_t lse_bytes = with_lse_out ? 0 : round16((int64_t)sizeof(float) * num_nodes * H);
  const int64_t part_bytes = by_dst->num_split > 0 ? (int64_t)sizeof(float) * by_dst->num_items * 2 * H : 0;
  return lse_bytes + part_bytes;
}

extern "C" int het_rgat_attention_compact(const het_grouping* by_dst, const float* el_c, const float* er_c, int64_t H, double slope,
                                          const int64_t* col, const int64_t* srow, const int64_t* drow, const int64_t* eids,
                                          int64_t num_edges, int64_t num_nodes, float* lse_out, float* attn, void* workspace,
                                          int64_t workspace_bytes, het_stream stream) {
  const char* op = "het_rgat_attention_compact";
  hipStream_t s = (hipStream_t)stream;
  HET_REQUIRE(by_dst && num_edges >= 0 && num_nodes >= 0, "%s: null grouping or negative count", op);
  if (!attn_heads_ok(H) || num_nodes >= (1ll << 31) || num_edges >= (1ll << 31)) {
    het_set_error("%s: unsupported shape H=%lld N=%lld E=%lld (1, 2, 4 or 8 heads, int32 node and edge counts)", op, (long long)H,
                  (long long)num_nodes, (long long)num_edges);
    return HET_ERR_UNSUPPORTED;
  }
  if (num_edges == 0) {
    HET_REQUIRE(by_dst->E == 0, "%s: by_dst groups %lld positions, num_edges is 0", op, (long long)by_dst->E);
    return HET_OK;  // (nothing touched)
  }
  HET_REQUIRE(el_c && er_c && col && srow && drow && attn, "%s: null argument (el_c, er_c, col, srow, drow and attn are required)", op);
  HET_REQUIRE(aligned16(el_c, er_c, attn, lse_out) && ((reinterpret_cast<uintptr_t>(col) | reinterpret_cast<uintptr_t>(srow) |
                                                        reinterpret_cast<uintptr_t>(drow) | reinterpret_cast<uintptr_t>(eids)) & 7) == 0,
              "%s: misaligned argument (el_c, er_c, attn, lse_out: 16 bytes; the id lists: 8)", op);
  HET_REQUIRE(by_dst->R == 0 && by_dst->E == num_edges && by_dst->key_bound <= num_nodes && by_dst->p0 && by_dst->p1,
              "%s: by_dst must group the %lld positions by destination (< num_nodes) with payload0 = feat row and payload1 = er row", op,
              (long long)num_edges);
  const int64_t need = het_rgat_attention_compact_workspace(by_dst, H, num_nodes, lse_out != nullptr);
  HET_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && aligned16(workspace)),
              "%s: a 16-byte aligned workspace of %lld bytes is needed (het_rgat_attention_compact_workspace)", op, (long long)need);
  const bool by_dst_order = attn_by_dst();
  if (by_dst_order)
    if (int rc = grouping_packs(by_dst, s)) return rc;  // (key_of_rank)
  float* lse = lse_out;
  char* ws = static_cast<char*>(workspace);
  if (!lse) {  // (scratch rows of destinations without in-edges stay unwritten: no edge reads them)
    lse = reinterpret_cast<float*>(ws);
    ws += round16((int64_t)sizeof(float) * num_nodes * H);
  } else {
    hipLaunchKernelGGL(HET_rgat_attn_fill, dim3(grid_for(num_nodes * H)), dim3(kBlock), 0, s, lse, num_nodes * H, -INFINITY);
    HET_LAUNCH_CHECK("HET_rgat_attn_fill");
  }
  float* part = reinterpret_cast<float*>(ws);
  const Items it = items_of(by_dst);
  {
    HET_KTIME("HET_rgat_attn_lse", s);
    const int64_t ipb = (int64_t)(kBlock / 64) * (H == 8 ? 4 : 8);  // items per workgroup (HET_rgat_attn_lse: IPW)
    const unsigned nb = (unsigned)ceil_div64(by_dst->num_items, ipb);
    HET_DISPATCH_HEADS((int)H, hipLaunchKernelGGL(HET_rgat_attn_lse<H>, dim3(nb), dim3(kBlock), 0, s, it, by_dst->p0, by_dst->p1, el_c,
                                                  er_c, (float)slope, lse, part));
    HET_LAUNCH_CHECK("HET_rgat_attn_lse");
    if (by_dst->num_split > 0) {
      const unsigned nbs = (unsigned)ceil_div64(by_dst->num_split, kBlock / 64);
      HET_DISPATCH_HEADS((int)H, hipLaunchKernelGGL(HET_rgat_attn_lse_finish<H>, dim3(nbs), dim3(kBlock), 0, s, by_dst->split_seg,
                                                    by_dst->num_split, it, part, lse));
      HET_LAUNCH_CHECK("HET_rgat_attn_lse_finish");
    }
  }
  {
    HET_KTIME("HET_rgat_attn_rows", s);
    const unsigned nb = (unsigned)ceil_div64(num_edges * (H == 8 ? 2 : 1), kBlock);
    if (by_dst_order) {
      HET_DISPATCH_HEADS((int)H, hipLaunchKernelGGL(HET_rgat_attn_rows_by_dst<H>, dim3(nb), dim3(kBlock), 0, s, by_dst->key_of_rank,
                                                    by_dst->p0, by_dst->p1, by_dst->perm, eids, num_edges, el_c, er_c, lse,
                                                    (float)slope, attn));
    } else {
      HET_DISPATCH_HEADS((int)H, hipLaunchKernelGGL(HET_rgat_attn_rows<H>, dim3(nb), dim3(kBlock), 0, s, col, srow, drow, eids,
                                                    num_edges, el_c, er_c, lse, (float)slope, attn));
    }
    HET_LAUNCH_CHECK("HET_rgat_attn_rows");
  }
  return HET_OK;
}
