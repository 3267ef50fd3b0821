// HGT edge softmax and message mean aggregation on the CSR layouts, forward and backward: the reference's IntegratedCSR ops
// (HGTOps.inc.h:23-106 switch 3, 109-188 switch 1, 282-325, 410-487 switch 2, 489-566 switch 2) that its unfused HGT path calls
// (hgt_layers_and_funcs.py:298-422).
//
// Fast paths walk a grouping of the CSR positions by destination (payload0 = edge id, payload1 = relation of the position):
// a wave per work item, a lane group per edge, so a destination is a segmented reduction in registers and a hub destination
// (more than HET_ITEM_MAX in-edges) is split over several work items.  Only the partial sums of split segments meet in global
// memory (float atomics on a zero-filled [N, H] / [N, H*dk] buffer, one per item and lane); the per-edge outputs of a split
// segment are finished by a second launch that reads the completed sums.  Without a grouping, or for other shapes, the
// plain kernels below run a thread per (destination, head) / (position, head) / (position, feature).
#include "coop.hip.h"
#include "grouping.hip.h"

namespace {

constexpr int kMaxLdsSlots = 64 * 64;  // (relation, head) partial sums of grad_mu reduced in LDS

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// a grouping of exactly these E positions by destination alone, carrying the edge id (and the relation when `need_rel`)
inline bool dst_grouping_ok(const het_grouping* g, int64_t E, bool need_rel) {
  return g && g->R == 0 && g->E == E && g->p0 && (!need_rel || g->p1);
}
// float4 per lane over the H heads of a score row
inline bool heads_shape_ok(int64_t H) { return H % 4 == 0 && is_pow2(H / 4) && H / 4 <= 64; }
// float4 per lane over the X = H*dk features of a message row; the dk/4 lanes of a head combine with head_sum (<= 32 lanes)
inline bool rows_shape_ok(int64_t H, int64_t dk) {
  const int64_t X = H * dk;
  return dk >= 4 && dk <= 128 && is_pow2(dk) && is_pow2(X) && X >= 8 && X <= 256;
}

#define HET_CSR_DL(DLV, CALL)                           \
  switch (DLV) {                                        \
    case 1: { constexpr int DL = 1; CALL; break; }      \
    case 2: { constexpr int DL = 2; CALL; break; }      \
    case 4: { constexpr int DL = 4; CALL; break; }      \
    case 8: { constexpr int DL = 8; CALL; break; }      \
    case 16: { constexpr int DL = 16; CALL; break; }    \
    default: { constexpr int DL = 32; CALL; break; }    \
  }

// ---- the two per-destination softmax passes ---------------------------------------------------------------------------
// MODE 0 (softmax forward):  val = exp(score[eid] * mu[rel]);  total = SUM over the in-edges of val  (-> sum[v]);
//                            then m[eid] = val, a[eid] = val / total
// MODE 1 (enorm backward):   val = a[eid] * grad_a[eid];       total = SUM over the in-edges of val;
//                            then c = (grad_a - total) * a,  grad_score[eid] = c * mu[rel],  grad_mu[rel] += c * score[eid]
struct SoftmaxArgs {
  const float *score, *mu, *a, *grad_a;
  float* total;  // [N, H]: sum (MODE 0), or a workspace for split destinations (MODE 1); zero-filled where atomics land
  float *m, *a_out, *grad_score, *grad_mu;
  int R;
};

template <int MODE>
__device__ __forceinline__ float4 softmax_val(const SoftmaxArgs& p, int64_t eid, int rel, int H, int x) {
  if (MODE == 0) {
    const float4 s = ld4(p.score + eid * H + x), mv = ld4(p.mu + (int64_t)rel * H + x);
    return make_float4(expf(s.x * mv.x), expf(s.y * mv.y), expf(s.z * mv.z), expf(s.w * mv.w));
  }
  const float4 a = ld4(p.a + eid * H + x), g = ld4(p.grad_a + eid * H + x);
  return make_float4(a.x * g.x, a.y * g.y, a.z * g.z, a.w * g.w);
}

// Wave per work item, H/4 lanes x float4 per edge, U edges per lane group in flight.  SPLIT_PASS = false: every item adds up its
// edges; a whole-segment item then finishes its edges at once, a split item adds its partial sum into p.total.  SPLIT_PASS =
// true (launched after): split items finish their edges with the completed p.total[v].  MODE 1 reduces grad_mu over the block in
// LDS ([R, H]) and flushes one atomic per (relation, head) and block.
template <int LPR, int MODE, bool SPLIT_PASS>
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_softmax_items(Items it, const int32_t* __restrict__ p_eid,
                                                                     const int32_t* __restrict__ p_rel, SoftmaxArgs p) {
  constexpr int EPW = 64 / LPR, H = LPR * 4, U = 4;
  extern __shared__ float part[];  // [R * H] (MODE 1)
  if (MODE == 1) {
    for (int i = threadIdx.x; i < p.R * H; i += kBlock) part[i] = 0.f;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, slot = lane / LPR, x = (lane % LPR) * 4;
  const int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (item < it.n) {
    const int seg = it.seg[item], b = it.begin[item], e = it.end[item];
    const bool whole = b == it.seg_ptr[seg] && e == it.seg_ptr[seg + 1];
    const int64_t v = it.seg_key[seg];
    if (!SPLIT_PASS || !whole) {
      float4 tot;
      if (SPLIT_PASS) {
        tot = ld4(p.total + v * H + x);
      } else {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j0 = b + slot; j0 < e; j0 += EPW * U) {
          int64_t eid[U];
          int rl[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int j = j0 + u * EPW, jc = j < e ? j : e - 1;
            eid[u] = p_eid[jc];
            rl[u] = MODE == 0 ? p_rel[jc] : 0;
          }
          float4 val[U];
#pragma unroll
          for (int u = 0; u < U; ++u) val[u] = softmax_val<MODE>(p, eid[u], rl[u], H, x);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float ok = j0 + u * EPW < e ? 1.f : 0.f;
            acc.x += ok * val[u].x; acc.y += ok * val[u].y; acc.z += ok * val[u].z; acc.w += ok * val[u].w;
          }
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
          acc.x += __shfl_xor(acc.x, off); acc.y += __shfl_xor(acc.y, off);
          acc.z += __shfl_xor(acc.z, off); acc.w += __shfl_xor(acc.w, off);
        }
        tot = acc;
        if (slot == 0) {
          if (!whole) atomic_add4(p.total + v * H + x, acc);  // hub destination: partial sum
          else if (MODE == 0) st4(p.total + v * H + x, acc);
        }
      }
      if (SPLIT_PASS || whole) {
        for (int j0 = b + slot; j0 < e; j0 += EPW * U) {
          int64_t eid[U];
          int rl[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int j = j0 + u * EPW, jc = j < e ? j : e - 1;
            eid[u] = p_eid[jc];
            rl[u] = p_rel[jc];
          }
          if (MODE == 0) {
            float4 val[U];
#pragma unroll
            for (int u = 0; u < U; ++u) val[u] = softmax_val<0>(p, eid[u], rl[u], H, x);
#pragma unroll
            for (int u = 0; u < U; ++u) {
              if (j0 + u * EPW >= e) continue;
              st4(p.m + eid[u] * H + x, val[u]);
              st4(p.a_out + eid[u] * H + x, make_float4(val[u].x / tot.x, val[u].y / tot.y, val[u].z / tot.z, val[u].w / tot.w));
            }
          } else {
            float4 av[U], ga[U], sc[U], mv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              av[u] = ld4(p.a + eid[u] * H + x);
              ga[u] = ld4(p.grad_a + eid[u] * H + x);
              sc[u] = ld4(p.score + eid[u] * H + x);
              mv[u] = ld4(p.mu + (int64_t)rl[u] * H + x);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
              if (j0 + u * EPW >= e) continue;
              const float4 c = make_float4((ga[u].x - tot.x) * av[u].x, (ga[u].y - tot.y) * av[u].y, (ga[u].z - tot.z) * av[u].z,
                                           (ga[u].w - tot.w) * av[u].w);
              st4(p.grad_score + eid[u] * H + x, make_float4(c.x * mv[u].x, c.y * mv[u].y, c.z * mv[u].z, c.w * mv[u].w));
              float* q = part + rl[u] * H + x;
              atomicAdd(q + 0, c.x * sc[u].x); atomicAdd(q + 1, c.y * sc[u].y);
              atomicAdd(q + 2, c.z * sc[u].z); atomicAdd(q + 3, c.w * sc[u].w);
            }
          }
        }
      }
    }
  }
  if (MODE == 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < p.R * H; i += kBlock)
      if (part[i] != 0.f) atomicAdd(&p.grad_mu[i], part[i]);
  }
}

// Plain form, any H: a thread per (destination, head) walks the destination's in-CSR row twice (no atomics but grad_mu's).
template <int MODE>
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_softmax_plain(const idx_t* __restrict__ row_ptr, const idx_t* __restrict__ eids,
                                                                     const idx_t* __restrict__ rel, int64_t N, int H, SoftmaxArgs p) {
  const int64_t total = N * H, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
    const int64_t v = t / H;
    const int h = (int)(t - v * H);
    const idx_t b = row_ptr[v], e = row_ptr[v + 1];
    float tot = 0.f;
    for (idx_t j = b; j < e; ++j) {
      const int64_t k = eids[j] * H + h;
      tot += MODE == 0 ? expf(p.score[k] * p.mu[rel[j] * H + h]) : p.a[k] * p.grad_a[k];
    }
    if (MODE == 0) p.total[t] = tot;
    for (idx_t j = b; j < e; ++j) {
      const int64_t k = eids[j] * H + h, km = rel[j] * H + h;
      if (MODE == 0) {
        const float val = expf(p.score[k] * p.mu[km]);
        p.m[k] = val;
        p.a_out[k] = val / tot;
      } else {
        const float c = (p.grad_a[k] - tot) * p.a[k];
        p.grad_score[k] = c * p.mu[km];
        atomicAdd(&p.grad_mu[km], c * p.score[k]);
      }
    }
  }
}

// ---- aggregation forward: ret[v] = SUM over the in-edges of attn[eid] / sum[v] * msg[eid] -----------------------------------
// Wave per work item, X/4 lanes x float4 per edge (X = H*dk), U edges per lane group in flight; the 1/sum[v] factor is applied
// once to the destination's total.  With DL = dk/4 >= 4 lanes per head, lane (head h, d < 4) fetches the edge id and the
// score of edge d of a step and the head's lanes share them (coop.hip.h); narrower heads load them per lane.
template <int LPR, int DL>
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_aggregate_items(Items it, const int32_t* __restrict__ p_eid,
                                                                       const float* __restrict__ msg,
                                                                       const float* __restrict__ attn,
                                                                       const float* __restrict__ sum, float* __restrict__ ret,
                                                                       int H) {
  constexpr int EPW = 64 / LPR, X = LPR * 4, U = 4;
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, sub = lane % LPR, x = sub * 4, h = sub / DL, d = sub % DL;
  const int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (item >= it.n) return;
  const int seg = it.seg[item], b = it.begin[item], e = it.end[item];
  const int64_t v = it.seg_key[seg];
  const bool whole = b == it.seg_ptr[seg] && e == it.seg_ptr[seg + 1];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j0 = b + slot; j0 < e; j0 += EPW * U) {
    int64_t eid[U];
    float w[U];
    if constexpr (DL >= U) {
      const int dq = d < U ? d : U - 1, jq = j0 + dq * EPW, jc = jq < e ? jq : e - 1;
      const int eidv = p_eid[jc];
      const float wv = jq < e ? attn[(int64_t)eidv * H + h] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {  // (all lanes of a head share the trip count: the broadcasts see active lanes only)
        eid[u] = head_bcast_i<DL>(eidv, u, lane);
        w[u] = head_bcast<DL>(wv, u, lane);
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u * EPW, jc = j < e ? j : e - 1;
        eid[u] = p_eid[jc];
        w[u] = j < e ? attn[eid[u] * H + h] : 0.f;
      }
    }
    float4 f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) f[u] = ld4(msg + eid[u] * X + x);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc.x = fmaf(w[u], f[u].x, acc.x); acc.y = fmaf(w[u], f[u].y, acc.y);
      acc.z = fmaf(w[u], f[u].z, acc.z); acc.w = fmaf(w[u], f[u].w, acc.w);
    }
  }
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off); acc.y += __shfl_xor(acc.y, off);
    acc.z += __shfl_xor(acc.z, off); acc.w += __shfl_xor(acc.w, off);
  }
  if (slot != 0) return;
  const float inv = 1.f / sum[v * H + h];
  const float4 r = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  if (whole) st4(ret + v * X + x, r);
  else atomic_add4(ret + v * X + x, r);  // hub destination: ret is zero-filled by the caller
}

// plain form, any shape: a thread per (destination, feature)
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_aggregate_plain(const idx_t* __restrict__ row_ptr, const idx_t* __restrict__ eids,
                                                                       int64_t N, const float* __restrict__ msg,
                                                                       const float* __restrict__ attn, const float* __restrict__ sum,
                                                                       float* __restrict__ ret, int H, int D) {
  const int X = H * D;
  const int64_t total = N * X, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
    const int64_t v = t / X;
    const int xx = (int)(t - v * X), h = xx / D;
    const idx_t b = row_ptr[v], e = row_ptr[v + 1];
    float acc = 0.f;
    for (idx_t j = b; j < e; ++j) acc = fmaf(attn[eids[j] * H + h], msg[eids[j] * X + xx], acc);
    ret[t] = b < e ? acc / sum[v * H + h] : 0.f;
  }
}

// ---- message backward: grad_message[eid] = a[eid] * gradout[col] over the out-CSR positions (a map, one store per row) --------
template <int LPR>
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_message_bwd_rows(const idx_t* __restrict__ col, const idx_t* __restrict__ eids,
                                                                        int64_t E, const float* __restrict__ a,
                                                                        const float* __restrict__ gradout,
                                                                        float* __restrict__ grad_msg, int H, int D) {
  constexpr int GPB = kBlock / LPR, X = LPR * 4, U = 4;  // lane groups per block
  const int grp = threadIdx.x / LPR, x = (threadIdx.x % LPR) * 4, h = x / D;
  const int64_t step = (int64_t)gridDim.x * GPB * U;
  for (int64_t base = (int64_t)blockIdx.x * GPB * U; base < E; base += step) {
    int64_t eid[U], ds[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * GPB + grp;
      ok[u] = i < E;
      const int64_t ic = ok[u] ? i : E - 1;
      eid[u] = eids[ic];
      ds[u] = col[ic];
    }
    float w[U];
    float4 g[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = a[eid[u] * H + h];
#pragma unroll
    for (int u = 0; u < U; ++u) g[u] = ld4(gradout + ds[u] * X + x);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u]) st4(grad_msg + eid[u] * X + x, make_float4(w[u] * g[u].x, w[u] * g[u].y, w[u] * g[u].z, w[u] * g[u].w));
  }
}

__global__ __launch_bounds__(kBlock) void HET_hgt_csr_message_bwd_plain(const idx_t* __restrict__ col, const idx_t* __restrict__ eids,
                                                                         int64_t E, const float* __restrict__ a,
                                                                         const float* __restrict__ gradout,
                                                                         float* __restrict__ grad_msg, int H, int D) {
  const int X = H * D;
  const int64_t total = E * X, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / X;
    const int xx = (int)(t - i * X);
    const int64_t eid = eids[i];
    grad_msg[eid * X + xx] = a[eid * H + xx / D] * gradout[col[i] * X + xx];
  }
}

// ---- softmax backward: c = a * <gradout[v], msg[eid] - out[v]> per head;  grad_score = mu[rel] * c;  grad_mu[rel] += c * score
// Destination-major over the out-CSR positions (a grouping by col): a wave per work item holds its destination's gradout / out
// rows in registers and takes <gradout[v], out[v]> once, then streams the message rows of the destination's edges.  grad_mu is
// reduced in LDS ([R, H]) and flushed with one atomic per (relation, head) and block.
template <int LPR, int DL>
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_softmax_bwd_items(Items it, const int32_t* __restrict__ p_eid,
                                                                         const int32_t* __restrict__ p_rel,
                                                                         const float* __restrict__ msg,
                                                                         const float* __restrict__ score,
                                                                         const float* __restrict__ a,
                                                                         const float* __restrict__ out,
                                                                         const float* __restrict__ gradout,
                                                                         const float* __restrict__ mu,
                                                                         float* __restrict__ grad_score,
                                                                         float* __restrict__ grad_mu, int H, int R) {
  constexpr int EPW = 64 / LPR, X = LPR * 4, U = 4;
  extern __shared__ float part[];  // [R * H]
  for (int i = threadIdx.x; i < R * H; i += kBlock) part[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int slot = lane / LPR, sub = lane % LPR, x = sub * 4, h = sub / DL, d = sub % DL;
  const int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (item < it.n) {
    const int seg = it.seg[item], b = it.begin[item], e = it.end[item];
    const int64_t v = it.seg_key[seg];
    const float4 g = ld4(gradout + v * X + x);
    const float go = head_sum<DL>(dot4(g, ld4(out + v * X + x)));
    for (int j0 = b + slot; j0 < e; j0 += EPW * U) {
      int64_t eid[U];
      int rl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u * EPW, jc = j < e ? j : e - 1;
        eid[u] = p_eid[jc];
        rl[u] = p_rel[jc];
      }
      float4 f[U];
      float av[U], sv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) f[u] = ld4(msg + eid[u] * X + x);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        av[u] = a[eid[u] * H + h];
        sv[u] = score[eid[u] * H + h];
        mv[u] = mu[(int64_t)rl[u] * H + h];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float c = av[u] * (head_sum<DL>(dot4(g, f[u])) - go);  // (outside the branch: head_sum reads the head's lanes)
        if (j0 + u * EPW < e && d == 0) {
          grad_score[eid[u] * H + h] = c * mv[u];
          atomicAdd(&part[rl[u] * H + h], c * sv[u]);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < R * H; i += kBlock)
    if (part[i] != 0.f) atomicAdd(&grad_mu[i], part[i]);
}

// plain form, any shape: a thread per (out-CSR position, head)
__global__ __launch_bounds__(kBlock) void HET_hgt_csr_softmax_bwd_plain(const idx_t* __restrict__ col, const idx_t* __restrict__ eids,
                                                                         const idx_t* __restrict__ rel, int64_t E,
                                                                         const float* __restrict__ msg,
                                                                         const float* __restrict__ score,
                                                                         const float* __restrict__ a, const float* __restrict__ out,
                                                                         const float* __restrict__ gradout,
                                                                         const float* __restrict__ mu, float* __restrict__ grad_score,
                                                                         float* __restrict__ grad_mu, int H, int D) {
  const int64_t total = E * H, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / H;
    const int h = (int)(t - i * H);
    const int64_t eid = eids[i], v = col[i], k = eid * H + h, km = rel[i] * H + h;
    const float* m = msg + k * D;
    const float* o = out + (v * H + h) * D;
    const float* g = gradout + (v * H + h) * D;
    float s = 0.f;
    for (int dd = 0; dd < D; ++dd) s = fmaf(g[dd], m[dd] - o[dd], s);
    const float c = a[k] * s;
    grad_score[k] = c * mu[km];
    atomicAdd(&grad_mu[km], c * score[k]);
  }
}

int check_csr(const char* op, const idx_t* row_ptrs, int64_t row_ptrs_len, const idx_t* col, const idx_t* eids, const idx_t* rel,
              int64_t num_nodes, int64_t num_edges) {
  HET_REQUIRE(num_nodes >= 0 && num_edges >= 0 && num_nodes < (1ll << 31) && num_edges < (1ll << 31), "%s: bad sizes", op);
  HET_REQUIRE(row_ptrs_len == num_nodes + 1, "%s: row_ptrs has %lld entries, expected num_nodes + 1 = %lld", op,
              (long long)row_ptrs_len, (long long)(num_nodes + 1));
  HET_REQUIRE(row_ptrs && (num_edges == 0 || (col && eids && rel)), "%s: null index pointer", op);
  return HET_OK;
}

int launch_softmax_items(int mode, const het_grouping* g, int64_t H, const SoftmaxArgs& p, hipStream_t s) {
  const unsigned nb = (unsigned)ceil_div64(g->num_items, kBlock / 64);
  const size_t lds = mode == 1 ? sizeof(float) * p.R * H : 0;
  const Items it = items_of(g);
#define HET_SM(MODEV, SPLIT) HET_DISPATCH_LPR((int)(H / 4), hipLaunchKernelGGL((HET_hgt_csr_softmax_items<LPR, MODEV, SPLIT>), dim3(nb), \
                                                                           dim3(kBlock), lds, s, it, g->p0, g->p1, p))
  if (mode == 0) { HET_SM(0, false); } else { HET_SM(1, false); }
  HET_LAUNCH_CHECK("HET_hgt_csr_softmax_items");
  if (g->num_split > 0) {  // hub destinations: their edges once the partial sums are complete
    if (mode == 0) { HET_SM(0, true); } else { HET_SM(1, true); }
    HET_LAUNCH_CHECK("HET_hgt_csr_softmax_items");
  }
#undef HET_SM
  return HET_OK;
}

}  // namespace

extern "C" int het_hgt_full_graph_edge_softmax_ops_csr(const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices,
                                                       const int64_t* eids, const int64_t* reltypes, int64_t num_nodes,
                                                       int64_t num_edges, const float* score, const float* mu, float* sum,
                                                       float* m, float* a, int64_t H, const het_grouping* by_dst,
                                                       het_stream stream) {
  const char* op = "hgt_full_graph_edge_softmax_ops_csr";
  if (int rc = check_csr(op, row_ptrs, row_ptrs_len, col_indices, eids, reltypes, num_nodes, num_edges)) return rc;
  HET_REQUIRE(H > 0 && (num_nodes == 0 || sum) && (num_edges == 0 || (score && mu && m && a)), "%s: null data pointer", op);
  hipStream_t s = (hipStream_t)stream;
  SoftmaxArgs p{score, mu, nullptr, nullptr, sum, m, a, nullptr, nullptr, 0};
  if (num_edges > 0 && dst_grouping_ok(by_dst, num_edges, true) && heads_shape_ok(H) && aligned16(score, mu, sum, m, a)) {
    HET_HIP(hipMemsetAsync(sum, 0, sizeof(float) * num_nodes * H, s));  // (destinations without in-edges; hub partial sums)
    return launch_softmax_items(0, by_dst, H, p, s);
  }
  if (num_nodes == 0) return HET_OK;
  hipLaunchKernelGGL(HET_hgt_csr_softmax_plain<0>, dim3(grid_for(num_nodes * H)), dim3(kBlock), 0, s, row_ptrs, eids, reltypes,
                     num_nodes, (int)H, p);
  HET_LAUNCH_CHECK("HET_hgt_csr_softmax_plain");
  return HET_OK;
}

extern "C" int het_hgt_full_graph_message_mean_aggregation_csr(const int64_t* row_ptrs, int64_t row_ptrs_len,
                                                               const int64_t* col_indices, const int64_t* reltypes,
                                                               const int64_t* eids, int64_t num_nodes, int64_t num_edges,
                                                               const float* edge_messages, const float* edge_attn_score,
                                                               const float* sum, const float* mu, float* ret, int64_t H,
                                                               int64_t dk, const het_grouping* by_dst, het_stream stream) {
  const char* op = "hgt_full_graph_message_mean_aggregation_csr";
  if (int rc = check_csr(op, row_ptrs, row_ptrs_len, col_indices, eids, reltypes, num_nodes, num_edges)) return rc;
  HET_REQUIRE(H > 0 && dk > 0 && (num_nodes == 0 || ret) && (num_edges == 0 || (edge_messages && edge_attn_score && sum)),
              "%s: null data pointer", op);
  (void)mu;  // switch 1: the score is mu-applied already
  hipStream_t s = (hipStream_t)stream;
  if (num_edges > 0 && dst_grouping_ok(by_dst, num_edges, false) && rows_shape_ok(H, dk) && aligned16(edge_messages, ret)) {
    HET_HIP(hipMemsetAsync(ret, 0, sizeof(float) * num_nodes * H * dk, s));
    const het_grouping* g = by_dst;
    const unsigned nb = (unsigned)ceil_div64(g->num_items, kBlock / 64);
    const Items it = items_of(g);
    HET_DISPATCH_LPR((int)(H * dk / 4), HET_CSR_DL((int)(dk / 4), hipLaunchKernelGGL((HET_hgt_csr_aggregate_items<LPR, DL>), dim3(nb),
                                                                                 dim3(kBlock), 0, s, it, g->p0, edge_messages,
                                                                                 edge_attn_score, sum, ret, (int)H)));
    HET_LAUNCH_CHECK("HET_hgt_csr_aggregate_items");
    return HET_OK;
  }
  if (num_nodes == 0) return HET_OK;
  hipLaunchKernelGGL(HET_hgt_csr_aggregate_plain, dim3(grid_for(num_nodes * H * dk)), dim3(kBlock), 0, s, row_ptrs, eids, num_nodes,
                     edge_messages, edge_attn_score, sum, ret, (int)H, (int)dk);
  HET_LAUNCH_CHECK("HET_hgt_csr_aggregate_plain");
  return HET_OK;
}

extern "C" int het_backward_hgt_full_graph_message_mean_aggregation_csr(
    const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices, const int64_t* reltypes, const int64_t* eids,
    int64_t num_nodes, int64_t num_edges, const float* sum, const float* normalized_attn_score, const float* gradout,
    float* grad_message, int64_t H, int64_t dk, het_stream stream) {
  const char* op = "backward_hgt_full_graph_message_mean_aggregation_csr";
  if (int rc = check_csr(op, row_ptrs, row_ptrs_len, col_indices, eids, reltypes, num_nodes, num_edges)) return rc;
  HET_REQUIRE(H > 0 && dk > 0 && (num_edges == 0 || (normalized_attn_score && gradout && grad_message)), "%s: null data pointer", op);
  (void)sum;  // switch 2: the normalised score is given
  if (num_edges == 0) return HET_OK;
  hipStream_t s = (hipStream_t)stream;
  if (rows_shape_ok(H, dk) && aligned16(gradout, grad_message)) {
    const int lpr = (int)(H * dk / 4);
    const unsigned nb = grid_for(ceil_div64(num_edges * lpr, 4));
    HET_DISPATCH_LPR(lpr, hipLaunchKernelGGL(HET_hgt_csr_message_bwd_rows<LPR>, dim3(nb), dim3(kBlock), 0, s, col_indices, eids, num_edges,
                                        normalized_attn_score, gradout, grad_message, (int)H, (int)dk));
    HET_LAUNCH_CHECK("HET_hgt_csr_message_bwd_rows");
    return HET_OK;
  }
  hipLaunchKernelGGL(HET_hgt_csr_message_bwd_plain, dim3(grid_for(num_edges * H * dk)), dim3(kBlock), 0, s, col_indices, eids,
                     num_edges, normalized_attn_score, gradout, grad_message, (int)H, (int)dk);
  HET_LAUNCH_CHECK("HET_hgt_csr_message_bwd_plain");
  return HET_OK;
}

extern "C" int het_backward_hgt_full_graph_edge_softmax_ops_csr(
    const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices, const int64_t* eids, const int64_t* reltypes,
    int64_t num_nodes, int64_t num_edges, int64_t num_rels, const float* message, const float* score,
    const float* normalized_attn_score, const float* out, const float* gradout, const float* mu, float* grad_attn_score,
    float* grad_mu, int64_t H, int64_t dk, const het_grouping* by_dst, het_stream stream) {
  const char* op = "backward_hgt_full_graph_edge_softmax_ops_csr";
  if (int rc = check_csr(op, row_ptrs, row_ptrs_len, col_indices, eids, reltypes, num_nodes, num_edges)) return rc;
  HET_REQUIRE(H > 0 && dk > 0 && num_rels > 0 &&
                  (num_edges == 0 || (message && score && normalized_attn_score && out && gradout && mu && grad_attn_score && grad_mu)),
              "%s: null data pointer", op);
  if (num_edges == 0) return HET_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dst_grouping_ok(by_dst, num_edges, true) && rows_shape_ok(H, dk) && num_rels * H <= kMaxLdsSlots &&
      aligned16(message, out, gradout)) {
    const het_grouping* g = by_dst;
    const unsigned nb = (unsigned)ceil_div64(g->num_items, kBlock / 64);
    const Items it = items_of(g);
    HET_DISPATCH_LPR((int)(H * dk / 4), HET_CSR_DL((int)(dk / 4), hipLaunchKernelGGL((HET_hgt_csr_softmax_bwd_items<LPR, DL>), dim3(nb),
                                                                                 dim3(kBlock), sizeof(float) * num_rels * H, s, it,
                                                                                 g->p0, g->p1, message, score,
                                                                                 normalized_attn_score, out, gradout, mu,
                                                                                 grad_attn_score, grad_mu, (int)H, (int)num_rels)));
    HET_LAUNCH_CHECK("HET_hgt_csr_softmax_bwd_items");
    return HET_OK;
  }
  hipLaunchKernelGGL(HET_hgt_csr_softmax_bwd_plain, dim3(grid_for(num_edges * H)), dim3(kBlock), 0, s, col_indices, eids, reltypes,
                     num_edges, message, score, normalized_attn_score, out, gradout, mu, grad_attn_score, grad_mu, (int)H, (int)dk);
  HET_LAUNCH_CHECK("HET_hgt_csr_softmax_bwd_plain");
  return HET_OK;
}

extern "C" int het_backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(
    const int64_t* row_ptrs, int64_t row_ptrs_len, const int64_t* col_indices, const int64_t* eids, const int64_t* reltypes,
    int64_t num_nodes, int64_t num_edges, int64_t num_rels, const float* score, const float* normalized_attn_score,
    const float* grad_normalized_attn_score, const float* mu, float* grad_score, float* grad_mu, int64_t H,
    const het_grouping* by_dst, void* workspace, int64_t workspace_bytes, het_stream stream) {
  const char* op = "backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr";
  if (int rc = check_csr(op, row_ptrs, row_ptrs_len, col_indices, eids, reltypes, num_nodes, num_edges)) return rc;
  HET_REQUIRE(H > 0 && num_rels > 0 &&
                  (num_edges == 0 || (score && normalized_attn_score && grad_normalized_attn_score && mu && grad_score && grad_mu)),
              "%s: null data pointer", op);
  if (num_edges == 0) return HET_OK;
  hipStream_t s = (hipStream_t)stream;
  SoftmaxArgs p{score, mu, normalized_attn_score, grad_normalized_attn_score, static_cast<float*>(workspace), nullptr, nullptr,
                grad_score, grad_mu, (int)num_rels};
  const het_grouping* g = by_dst;
  const bool ws_ok = g && (g->num_split == 0 || (workspace && workspace_bytes >= (int64_t)sizeof(float) * num_nodes * H &&
                                                 aligned16(workspace)));
  if (dst_grouping_ok(g, num_edges, true) && ws_ok && heads_shape_ok(H) && num_rels * H <= kMaxLdsSlots &&
      aligned16(score, mu, normalized_attn_score, grad_normalized_attn_score, grad_score)) {
    if (g->num_split > 0) HET_HIP(hipMemsetAsync(workspace, 0, sizeof(float) * num_nodes * H, s));
    return launch_softmax_items(1, g, H, p, s);
  }
  hipLaunchKernelGGL(HET_hgt_csr_softmax_plain<1>, dim3(grid_for(num_nodes * H)), dim3(kBlock), 0, s, row_ptrs, eids, reltypes,
                     num_nodes, (int)H, p);
  HET_LAUNCH_CHECK("HET_hgt_csr_softmax_plain");
  return HET_OK;
}
