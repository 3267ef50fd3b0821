// Filtered ranking of link-prediction queries against every node with the DistMult score (het_amd/linkpred.py distmult_rank; DESIGN.md
// 4.14; the rule in include/het_amd.h).  No score is stored: three integers per query come out.
//
// The rule (fp32; bf16 rows of h are widened first, which is exact):
//   query j = (a_j, r_j, t_j): anchor node, relation, true node.  [lo_j, hi_j) = the run of node_type_offsets that holds t_j ([0, N)
//   without offsets).  q_j[d] = fl32(h[a_j, d] * w[r_j, d]).  score_j(c) = the fp32 fma chain over ascending d from +0:
//   acc = fmaf(q_j[d], h[c, d], acc).  p_j = score_j(t_j) by the same chain.  Excluded: c == t_j and every listed pair (j, c); a pair
//   listed twice excludes once, a listed c outside the run changes nothing, a pair with an id outside its range is ignored.
//   greater_j / equal_j / cands_j = the number of c in the run, not excluded, with score_j(c) > p_j / == p_j / at all.
//   A query with a or t outside [0, N), r outside [0, R) or t in no run is BAD: counted, its three counts are 0 and no table is read
//   through its ids.
//
// ComplEx (het_complex_rank): the same pass behind HET_complex_rank_prelude, whose q_j follows the side of the query
// (the rule above rank_q_complex below); the pass never looks at w.
//
// Launches: HET_rank_prelude (one lane per query: the ids, the run, q_j, p_j as a sequential fmaf chain in plain C++, the three
// counters of the query set to zero, the bad queries counted with one integer atomic per wave into a counter an 8-byte memset
// cleared), HET_rank_pair_keys + one stable hipCUB radix sort of the listed pairs by the tile cell they fall in + HET_rank_tile_ptr
// (only when pairs are listed), HET_triple_rank (the pass below).  Nothing is read back and nothing waits for the stream.
//
// The pass.  A workgroup of 4 waves takes an item: a span of candidate tiles (kRankCandTile rows of h each) against a chunk of
// kRankChunkTiles query tiles (kRankQueryTile queries each).  A candidate tile is read from memory once (16-byte loads, bf16 widened
// on load) into LDS and multiplied against every query tile of the chunk; a query tile of q comes from the workspace (L2) into LDS.
// Each wave owns 32 queries x 32 candidates: 2 x 2 accumulators of v_mfma_f32_16x16x4_f32 (A = q, B = h: lane l feeds q[row l & 15]
// [4 kk + (l >> 4)] and h[row l & 15][4 kk + (l >> 4)] at step kk), which is bit for bit the fmaf chain of the rule.  The epilogue
// compares in registers against p_j, masks c outside [lo_j, hi_j), c == t_j and the bits of the tile's exclusion mask, counts with wave
// ballots into int32 LDS counters of the chunk, and adds the non-zero counters of the item into greater / equal / cands with integer
// atomics: the same bits on every call.  The exclusion masks of a candidate tile against every query tile of the chunk are set in LDS
// when the candidate tile is staged, from the tile's run of the sorted pairs (candidate tile major; HET_rank_tile_ptr finds every
// tile's run once, by binary search): setting a bit twice is harmless.  A query tile whose runs (their union, kept in LDS per item) do
// not meet the candidate tile is skipped before anything of it is loaded.  Every row offset is 64-bit.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "common.hip.h"

namespace {

constexpr int kRankQueryTile = 64;     // M: queries of a tile (2 waves x 2 MFMA row blocks of 16)
constexpr int kRankCandTile = 64;      // C: candidates of a tile (2 waves x 2 MFMA column blocks of 16)
constexpr int kRankMinWidth = 4;       // D is a multiple of 4 ...
constexpr int kRankMaxWidth = 256;     // ... up to this many columns (two [64, D + 4] fp32 tiles and the counters in 160 KB of LDS)
constexpr int kRankMaxBlocks = 4096;   // a workgroup takes further items beyond this many
constexpr int kRankChunkTiles = 16;    // query tiles whose counters a workgroup keeps in LDS
constexpr int kRankMaxSpan = 64;       // candidate tiles of an item at most
constexpr int kRankPad = 4;            // floats between the rows of an LDS tile (keeps them 16-byte aligned)
constexpr int64_t kRankMaxQueries = 1ll << 30, kRankMaxNodes = (1ll << 31) - 1, kRankMaxPairs = 1ll << 30;

typedef float rank_f4 __attribute__((ext_vector_type(4)));

bool rank_width_ok(int64_t d) { return d >= kRankMinWidth && d <= kRankMaxWidth && d % 4 == 0; }
int64_t rank_align256(int64_t b) { return (b + 255) & ~255ll; }
int rank_bits(uint64_t top) {  // bits that hold every value of [0, top]
  int b = 1;
  while (b < 64 && (1ull << b) <= top) ++b;
  return b;
}
size_t rank_lds_bytes(int64_t d) {
  return sizeof(float) * 2 * kRankQueryTile * (size_t)(d + kRankPad) + sizeof(int) * 3 * kRankChunkTiles * kRankQueryTile +
         4 * sizeof(int) * kRankQueryTile + sizeof(uint32_t) * kRankChunkTiles * kRankQueryTile * (kRankCandTile / 32) +
         2 * sizeof(int) * kRankChunkTiles;
}

// ---- prelude: one lane per query ----------------------------------------------------------------------------------------------------
// q of a piece.  DistMult: the rounded product.  ComplEx (column 2k the real, 2k + 1 the imaginary part; x = h[a_j], b = w[r_j]):
//   side 0 (tails are ranked, x stands for the head):  q[2k] = fl(fl(x_r b_r) - fl(x_i b_i))   q[2k+1] = fl(fl(x_r b_i) + fl(x_i b_r))
//   side 1 (heads are ranked, x stands for the tail):  q[2k] = fl(fl(b_r x_r) + fl(b_i x_i))   q[2k+1] = fl(fl(b_r x_i) - fl(b_i x_r))
// three separately rounded fp32 operations per element: nothing here may be contracted into a fused multiply-add
__device__ __forceinline__ float4 rank_q_distmult(const float4& x, const float4& y) {
  return make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w);
}
__device__ __forceinline__ float4 rank_q_complex(const float4& x, const float4& b, bool head) {
#pragma clang fp contract(off)  // (plain operators under the pragma: the products and the sums below carry no licence to fuse)
  const float rr0 = x.x * b.x, ii0 = x.y * b.y, ri0 = x.x * b.y, ir0 = x.y * b.x;
  const float rr1 = x.z * b.z, ii1 = x.w * b.w, ri1 = x.z * b.w, ir1 = x.w * b.z;
  if (head) return make_float4(rr0 + ii0, ir0 - ri0, rr1 + ii1, ir1 - ri1);
  return make_float4(rr0 - ii0, ri0 + ir0, rr1 - ii1, ri1 + ir1);
}

// the per-query work of both preludes: the ids, the run, the bad count, q_j and p_j, the zeroed counters.  CPX: side [nq] picks the
// ComplEx rule's q (a side outside {0, 1} makes the query bad); else side is not read.
template <typename T, bool CPX>
__device__ __forceinline__ void rank_prelude_body(const T* __restrict__ h, const float* __restrict__ w, const idx_t* __restrict__ a,
                                                  const idx_t* __restrict__ r, const idx_t* __restrict__ t, const idx_t* __restrict__ side,
                                                  idx_t nq, const idx_t* __restrict__ offs, int num_types, idx_t n, idx_t nr, idx_t d,
                                                  float* __restrict__ q, float* __restrict__ p, int* __restrict__ lo, int* __restrict__ hi,
                                                  int* __restrict__ tt, int* __restrict__ greater, int* __restrict__ equal,
                                                  int* __restrict__ cands, unsigned long long* __restrict__ bad) {
  const idx_t step = (idx_t)gridDim.x * kBlock, np = d >> 2;
  for (idx_t j0 = (idx_t)blockIdx.x * kBlock; j0 < nq; j0 += step) {  // (the same trip count in every lane of a wave: the ballot below)
    const idx_t j = j0 + threadIdx.x;
    const bool in = j < nq;
    idx_t aj = -1, rj = -1, tj = -1, sd = 0;
    if (in) {
      aj = a[j];
      rj = r[j];
      tj = t[j];
      if (CPX) sd = side[j];
    }
    bool ok = (uint64_t)aj < (uint64_t)n && (uint64_t)tj < (uint64_t)n && (uint64_t)rj < (uint64_t)nr && (uint64_t)sd < 2ull;
    idx_t l = 0, u = n;
    if (ok && offs) {
      ok = tj >= offs[0] && tj < offs[num_types];
      if (ok) {
        const int ty = find_segment(offs, num_types, tj);
        l = offs[ty] < 0 ? 0 : offs[ty];
        u = offs[ty + 1] > n ? n : offs[ty + 1];
      }
    }
    const unsigned long long badmask = __ballot(in && !ok);
    if ((threadIdx.x & (HET_WAVE - 1)) == 0 && badmask) atomicAdd(bad, (unsigned long long)__popcll(badmask));
    if (!in) continue;
    float acc = 0.f;
    float* qj = q + j * d;
    if (ok) {
      const T* ha = h + aj * d;
      const T* ht = h + tj * d;
      const float* wr = w + rj * d;
      for (idx_t pc = 0; pc < np; ++pc) {
        const float4 x = ldrow4(ha + 4 * pc), y = ld4(wr + 4 * pc), z = ldrow4(ht + 4 * pc);
        const float4 m = CPX ? rank_q_complex(x, y, sd != 0) : rank_q_distmult(x, y);
        st4(qj + 4 * pc, m);
        acc = fmaf(m.x, z.x, acc);
        acc = fmaf(m.y, z.y, acc);
        acc = fmaf(m.z, z.z, acc);
        acc = fmaf(m.w, z.w, acc);
      }
    } else {
      for (idx_t pc = 0; pc < np; ++pc) st4(qj + 4 * pc, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    p[j] = acc;
    lo[j] = ok ? (int)l : 0;
    hi[j] = ok ? (int)u : 0;
    tt[j] = ok ? (int)tj : -1;
    greater[j] = 0;
    equal[j] = 0;
    cands[j] = 0;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void HET_rank_prelude(const T* __restrict__ h, const float* __restrict__ w, const idx_t* __restrict__ a,
                                                           const idx_t* __restrict__ r, const idx_t* __restrict__ t, idx_t nq,
                                                           const idx_t* __restrict__ offs, int num_types, idx_t n, idx_t nr, idx_t d,
                                                           float* __restrict__ q, float* __restrict__ p, int* __restrict__ lo,
                                                           int* __restrict__ hi, int* __restrict__ tt, int* __restrict__ greater,
                                                           int* __restrict__ equal, int* __restrict__ cands,
                                                           unsigned long long* __restrict__ bad) {
  rank_prelude_body<T, false>(h, w, a, r, t, nullptr, nq, offs, num_types, n, nr, d, q, p, lo, hi, tt, greater, equal, cands, bad);
}

// the ComplEx prelude: the same work, q by the two-sided rule
template <typename T>
__global__ __launch_bounds__(kBlock) void HET_complex_rank_prelude(const T* __restrict__ h, const float* __restrict__ w,
                                                                   const idx_t* __restrict__ a, const idx_t* __restrict__ r,
                                                                   const idx_t* __restrict__ t, const idx_t* __restrict__ side, idx_t nq,
                                                                   const idx_t* __restrict__ offs, int num_types, idx_t n, idx_t nr, idx_t d,
                                                                   float* __restrict__ q, float* __restrict__ p, int* __restrict__ lo,
                                                                   int* __restrict__ hi, int* __restrict__ tt, int* __restrict__ greater,
                                                                   int* __restrict__ equal, int* __restrict__ cands,
                                                                   unsigned long long* __restrict__ bad) {
  rank_prelude_body<T, true>(h, w, a, r, t, side, nq, offs, num_types, n, nr, d, q, p, lo, hi, tt, greater, equal, cands, bad);
}

// ---- the listed pairs: the sort key is the tile cell, candidate tile major; a pair with an id outside its range sorts behind every cell
__global__ __launch_bounds__(kBlock) void HET_rank_pair_keys(const idx_t* __restrict__ pq, const idx_t* __restrict__ pc, idx_t npairs, idx_t nq,
                                                             idx_t n, idx_t nqt, idx_t nct, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ vals) {
  const idx_t step = (idx_t)gridDim.x * kBlock;
  for (idx_t i = (idx_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += step) {
    const idx_t qi = pq[i], ci = pc[i];
    const bool ok = (uint64_t)qi < (uint64_t)nq && (uint64_t)ci < (uint64_t)n;
    keys[i] = ok ? (uint64_t)(ci / kRankCandTile) * (uint64_t)nqt + (uint64_t)(qi / kRankQueryTile) : (uint64_t)nct * (uint64_t)nqt;
    vals[i] = ok ? (uint32_t)((qi % kRankQueryTile) * kRankCandTile + ci % kRankCandTile) : 0u;
  }
}

__device__ __forceinline__ idx_t rank_lower_bound(const uint64_t* __restrict__ k, idx_t lo, idx_t hi, uint64_t key) {
  while (lo < hi) {
    const idx_t mid = (lo + hi) >> 1;
    if (k[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// where the pairs of every candidate tile begin in the sorted keys: tile_ptr [nct + 1]
__global__ __launch_bounds__(kBlock) void HET_rank_tile_ptr(const uint64_t* __restrict__ keys, idx_t npairs, idx_t nqt, idx_t nct,
                                                            int* __restrict__ tile_ptr) {
  const idx_t step = (idx_t)gridDim.x * kBlock;
  for (idx_t ct = (idx_t)blockIdx.x * kBlock + threadIdx.x; ct <= nct; ct += step)
    tile_ptr[ct] = (int)rank_lower_bound(keys, 0, npairs, (uint64_t)ct * (uint64_t)nqt);
}

// ---- the rank pass -------------------------------------------------------------------------------------------------------------------
struct RankArgs {
  const float* q;       // [nq, d]
  const float* p;       // [nq]
  const int* lo;        // [nq]
  const int* hi;        // [nq]
  const int* tt;        // [nq]
  const uint64_t* keys; // [npairs] sorted cells
  const uint32_t* vals; // [npairs] (query in its tile) * C + (candidate in its tile)
  const int* tile_ptr;  // [nct + 1] the run of every candidate tile in keys / vals
  idx_t npairs, nq, n, d, nqt, nct, nqc, items;
  int span;
  int* greater;
  int* equal;
  int* cands;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void HET_triple_rank(const T* __restrict__ h, RankArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rank_lds[];
  const int S = (int)g.d + kRankPad, np = (int)(g.d >> 2);
  float* hs = reinterpret_cast<float*>(rank_lds);                 // [C][S]
  float* qs = hs + kRankCandTile * S;                             // [M][S]
  int* cnt = reinterpret_cast<int*>(qs + kRankQueryTile * S);     // [kRankChunkTiles * M][3]
  float* mp = reinterpret_cast<float*>(cnt + 3 * kRankChunkTiles * kRankQueryTile);  // [M]
  int* mlo = reinterpret_cast<int*>(mp + kRankQueryTile);         // [M]
  int* mhi = mlo + kRankQueryTile;                                // [M]
  int* mtt = mhi + kRankQueryTile;                                // [M]
  constexpr int kMaskWords = kRankChunkTiles * kRankQueryTile * (kRankCandTile / 32);
  uint32_t* mask = reinterpret_cast<uint32_t*>(mtt + kRankQueryTile);  // [kRankChunkTiles][M][C / 32]: the candidate tile's excluded pairs
  int* qr = reinterpret_cast<int*>(mask + kMaskWords);            // [kRankChunkTiles][2]: least lo and greatest hi of a query tile

  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lg = l >> 4, li = l & 15, wm = wave >> 1, wn = wave & 1;
  for (int i = tid; i < 3 * kRankChunkTiles * kRankQueryTile; i += kBlock) cnt[i] = 0;
  for (int i = tid; i < kMaskWords; i += kBlock) mask[i] = 0u;

  for (idx_t item = blockIdx.x; item < g.items; item += gridDim.x) {
    const idx_t sp = item / g.nqc, qc = item - sp * g.nqc;
    const idx_t ct0 = sp * g.span, ct1 = ct0 + g.span < g.nct ? ct0 + g.span : g.nct;
    const idx_t qt0 = qc * kRankChunkTiles, qt1 = qt0 + kRankChunkTiles < g.nqt ? qt0 + kRankChunkTiles : g.nqt;
    if (tid < 2 * kRankChunkTiles) qr[tid] = (tid & 1) ? 0 : 0x7fffffff;
    __syncthreads();
    for (int i = tid; i < (int)(qt1 - qt0) * kRankQueryTile; i += kBlock) {
      const idx_t j = qt0 * kRankQueryTile + i;
      if (j < g.nq) {
        const int a = g.lo[j], b = g.hi[j];
        if (b > a) {
          atomicMin(&qr[2 * (i / kRankQueryTile)], a);
          atomicMax(&qr[2 * (i / kRankQueryTile) + 1], b);
        }
      }
    }
    for (idx_t ct = ct0; ct < ct1; ++ct) {
      const idx_t c0 = ct * kRankCandTile;
      __syncthreads();  // the tile before this one has been multiplied
      for (int i = tid; i < kRankCandTile * np; i += kBlock) {
        const int row = i / np, pc = i - row * np;
        const idx_t c = c0 + row;
        const float4 v = c < g.n ? ldrow4(h + c * g.d + 4 * pc) : make_float4(0.f, 0.f, 0.f, 0.f);
        st4(hs + row * S + 4 * pc, v);
      }
      if (g.npairs) {
        for (int i = tid; i < kMaskWords; i += kBlock) mask[i] = 0u;
        __syncthreads();
        const int e = g.tile_ptr[ct + 1];
        for (int pos = g.tile_ptr[ct] + tid; pos < e; pos += kBlock) {
          const idx_t qtl = (idx_t)(g.keys[pos] - (uint64_t)ct * (uint64_t)g.nqt) - qt0;
          if (qtl < 0 || qtl >= qt1 - qt0) continue;
          const uint32_t v = g.vals[pos], ql = v / kRankCandTile, cl = v % kRankCandTile;
          if (ql < (uint32_t)kRankQueryTile)
            atomicOr(&mask[((int)qtl * kRankQueryTile + ql) * (kRankCandTile / 32) + (cl >> 5)], 1u << (cl & 31));
        }
      }
      for (idx_t qt = qt0; qt < qt1; ++qt) {
        const idx_t j0 = qt * kRankQueryTile;
        const int qtl = (int)(qt - qt0);
        if (!((idx_t)qr[2 * qtl] < c0 + kRankCandTile && (idx_t)qr[2 * qtl + 1] > c0)) continue;  // no query of the tile ranks in here
        __syncthreads();  // the query tile before this one has been multiplied; hs and the masks are written
        for (int i = tid; i < kRankQueryTile * np; i += kBlock) {
          const int row = i / np, pc = i - row * np;
          const idx_t j = j0 + row;
          const float4 v = j < g.nq ? ld4(g.q + j * g.d + 4 * pc) : make_float4(0.f, 0.f, 0.f, 0.f);
          st4(qs + row * S + 4 * pc, v);
        }
        if (tid < kRankQueryTile) {
          const idx_t j = j0 + tid;
          const bool in = j < g.nq;
          const int a = in ? g.lo[j] : 0, b = in ? g.hi[j] : 0;
          mp[tid] = in ? g.p[j] : 0.f;
          mlo[tid] = a;
          mhi[tid] = b;
          mtt[tid] = in ? g.tt[j] : -1;
        }
        __syncthreads();

        rank_f4 acc[2][2] = {};
        const float* qa = qs + (32 * wm + li) * S + lg;
        const float* hb = hs + (32 * wn + li) * S + lg;
        int kk = 0;
        for (; kk + 4 <= np; kk += 4) {  // four steps' operands in flight before the first of their 16 MFMAs
          float a0[4], a1[4], b0[4], b1[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            a0[u] = qa[4 * (kk + u)];
            a1[u] = qa[16 * S + 4 * (kk + u)];
            b0[u] = hb[4 * (kk + u)];
            b1[u] = hb[16 * S + 4 * (kk + u)];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b0[u], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b1[u], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b0[u], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b1[u], acc[1][1], 0, 0, 0);
          }
        }
        for (; kk < np; ++kk) {
          const float a0 = qa[4 * kk], a1 = qa[16 * S + 4 * kk], b0 = hb[4 * kk], b1 = hb[16 * S + 4 * kk];
          acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        // acc[ms][ns][v] = score(query 32 wm + 16 ms + 4 lg + v of the tile, candidate 32 wn + 16 ns + li of the tile); lane li of
        // each 16 keeps the counts of the query with 4 ms + v == li
        int ng = 0, ne = 0, nc = 0;
#pragma unroll
        for (int ms = 0; ms < 2; ++ms) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 32 * wm + 16 * ms + 4 * lg + v;
            const float pj = mp[row];
            const uint32_t a = (uint32_t)mlo[row], b = (uint32_t)mhi[row], tj = (uint32_t)mtt[row], bits = mask[(qtl * kRankQueryTile + row) * (kRankCandTile / 32) + wn];
#pragma unroll
            for (int ns = 0; ns < 2; ++ns) {
              const int cl = 16 * ns + li;
              const uint32_t c = (uint32_t)c0 + (uint32_t)(32 * wn + cl);
              const bool valid = c >= a && c < b && c != tj && !((bits >> cl) & 1u);
              const float s = acc[ms][ns][v];
              const unsigned long long bv = __ballot(valid), bg = __ballot(valid && s > pj), be = __ballot(valid && s == pj);
              if (li == 4 * ms + v) {
                nc += __popcll((bv >> (16 * lg)) & 0xffffull);
                ng += __popcll((bg >> (16 * lg)) & 0xffffull);
                ne += __popcll((be >> (16 * lg)) & 0xffffull);
              }
            }
          }
        }
        if (li < 8) {
          const int row = 32 * wm + 16 * (li >> 2) + 4 * lg + (li & 3);
          int* at = cnt + 3 * (qtl * kRankQueryTile + row);
          if (ng) atomicAdd(at, ng);
          if (ne) atomicAdd(at + 1, ne);
          if (nc) atomicAdd(at + 2, nc);
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < (int)(qt1 - qt0) * kRankQueryTile; i += kBlock) {
      const idx_t j = qt0 * kRankQueryTile + i;
      const int a = cnt[3 * i], b = cnt[3 * i + 1], c = cnt[3 * i + 2];
      cnt[3 * i] = 0;
      cnt[3 * i + 1] = 0;
      cnt[3 * i + 2] = 0;
      if (j < g.nq) {
        if (a) atomicAdd(g.greater + j, a);
        if (b) atomicAdd(g.equal + j, b);
        if (c) atomicAdd(g.cands + j, c);
      }
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct RankLayout {
  int64_t q, p, lo, hi, tt, keys_in, keys_out, vals_in, vals_out, tile_ptr, temp;
};
RankLayout rank_layout(int64_t nq, int64_t npairs, int64_t n, int64_t d) {
  RankLayout L;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t here = at; at += rank_align256(bytes); return here; };
  L.q = take(4 * nq * d);
  L.p = take(4 * nq);
  L.lo = take(4 * nq);
  L.hi = take(4 * nq);
  L.tt = take(4 * nq);
  L.keys_in = take(8 * npairs);
  L.keys_out = take(8 * npairs);
  L.vals_in = take(4 * npairs);
  L.vals_out = take(4 * npairs);
  L.tile_ptr = take(npairs ? 4 * (ceil_div64(n, kRankCandTile) + 1) : 0);
  L.temp = at;
  return L;
}

// bytes of hipCUB's own scratch for the sort of the pairs; 0 without pairs; -1 on failure
int64_t rank_temp_bytes(int64_t npairs, int bits) {
  if (npairs == 0) return 0;
  size_t b = 0;
  uint64_t* k = nullptr;
  uint32_t* v = nullptr;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, k, v, v, (int)npairs, 0, bits, (hipStream_t)0) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return rank_align256((int64_t)b);
}

int rank_check_sizes(const char* op, int64_t nq, int64_t npairs, int64_t d) {
  HET_REQUIRE(nq >= 0 && nq < kRankMaxQueries, "%s: num_queries=%lld (0 <= num_queries < 2^30)", op, (long long)nq);
  HET_REQUIRE(npairs >= 0 && npairs < kRankMaxPairs, "%s: num_pairs=%lld (0 <= num_pairs < 2^30)", op, (long long)npairs);
  HET_REQUIRE(d >= 1, "%s: dim=%lld (at least one column)", op, (long long)d);
  if (!rank_width_ok(d)) {
    het_set_error("%s: dim=%lld is not a width the kernels take (a multiple of 4 from %d to %d)", op, (long long)d, kRankMinWidth, kRankMaxWidth);
    return HET_ERR_UNSUPPORTED;
  }
  return HET_OK;
}

// complex_prelude: the ComplEx rule's q (side [nq]: 0 ranks tails, 1 ranks heads); everything behind the prelude is the same
template <typename T>
int triple_rank(const char* op, bool complex_prelude, const T* h, const float* w, const int64_t* a, const int64_t* r, const int64_t* t,
                const int64_t* side, int64_t nq, const int64_t* pq, const int64_t* pc, int64_t npairs, const int64_t* offs,
                int64_t num_types, int64_t n, int64_t nr, int64_t d,
                int32_t* greater, int32_t* equal, int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes, het_stream stream) {
  int rc = rank_check_sizes(op, nq, npairs, d);
  if (rc != HET_OK) return rc;
  HET_REQUIRE(n >= 0 && n < kRankMaxNodes, "%s: num_nodes=%lld (0 <= num_nodes < 2^31 - 1)", op, (long long)n);
  HET_REQUIRE(nr >= 0 && nr < kRankMaxNodes, "%s: num_rels=%lld (0 <= num_rels < 2^31 - 1)", op, (long long)nr);
  HET_REQUIRE(num_types >= 0 && num_types < kRankMaxNodes && (!offs || num_types >= 1), "%s: num_types=%lld%s", op, (long long)num_types,
              offs ? " with node_type_offsets (at least one run)" : "");
  if (nq == 0) return HET_OK;
  HET_REQUIRE(a && r && t && (side || !complex_prelude) && greater && equal && cands && bad && (h || n == 0) && (w || nr == 0) &&
                  (npairs == 0 || (pq && pc)),
              "%s: null pointer", op);
  HET_REQUIRE((sizeof(T) == 4 ? aligned16(h) : aligned8(h)) && aligned16(w, workspace) && aligned8(a, r, t, side, pq, pc, offs, bad) &&
                  (((uintptr_t)greater | (uintptr_t)equal | (uintptr_t)cands) & 3) == 0,
              "%s: misaligned pointer (h on %d-byte, w and workspace on 16-byte, int64 arrays on 8-byte, the counts on 4-byte boundaries)", op,
              (int)(4 * sizeof(T)));
  const RankLayout L = rank_layout(nq, npairs, n, d);
  HET_REQUIRE(workspace && workspace_bytes >= L.temp, "%s: workspace of %lld bytes, at least %lld needed (het_triple_rank_workspace)", op,
              (long long)(workspace ? workspace_bytes : 0), (long long)L.temp);
  const int64_t nqt = ceil_div64(nq, kRankQueryTile), nct = ceil_div64(n, kRankCandTile), nqc = ceil_div64(nqt, kRankChunkTiles);
  const int bits = rank_bits((uint64_t)nct * (uint64_t)nqt);
  const int64_t temp = rank_temp_bytes(npairs, bits);
  if (temp < 0) {
    het_set_error("%s: the sort's scratch size could not be asked", op);
    return HET_ERR_HIP;
  }
  HET_REQUIRE(workspace_bytes >= L.temp + temp, "%s: workspace of %lld bytes, %lld needed (het_triple_rank_workspace)", op,
              (long long)workspace_bytes, (long long)(L.temp + temp));
  const size_t lds = rank_lds_bytes(d);
  HET_REQUIRE(lds <= het_lds_budget(), "%s: dim=%lld needs %lld bytes of LDS, the device gives %lld", op, (long long)d, (long long)lds,
              (long long)het_lds_budget());
  char* base = (char*)workspace;
  float* q = (float*)(base + L.q);
  float* p = (float*)(base + L.p);
  int *lo = (int*)(base + L.lo), *hi = (int*)(base + L.hi), *tt = (int*)(base + L.tt);
  uint64_t *ki = (uint64_t*)(base + L.keys_in), *ko = (uint64_t*)(base + L.keys_out);
  uint32_t *vi = (uint32_t*)(base + L.vals_in), *vo = (uint32_t*)(base + L.vals_out);
  int* tile_ptr = (int*)(base + L.tile_ptr);
  hipStream_t st = (hipStream_t)stream;
  HET_HIP(hipMemsetAsync(bad, 0, sizeof(int64_t), st));
  if (complex_prelude) {
    HET_KTIME("HET_complex_rank_prelude", st);
    hipLaunchKernelGGL((HET_complex_rank_prelude<T>), dim3(grid_for(nq)), dim3(kBlock), 0, st, h, w, (const idx_t*)a, (const idx_t*)r,
                       (const idx_t*)t, (const idx_t*)side, (idx_t)nq, (const idx_t*)offs, (int)num_types, (idx_t)n, (idx_t)nr, (idx_t)d, q, p, lo,
                       hi, tt, greater, equal, cands, (unsigned long long*)bad);
    HET_LAUNCH_CHECK("HET_complex_rank_prelude");
  } else {
    HET_KTIME("HET_rank_prelude", st);
    hipLaunchKernelGGL((HET_rank_prelude<T>), dim3(grid_for(nq)), dim3(kBlock), 0, st, h, w, (const idx_t*)a, (const idx_t*)r, (const idx_t*)t,
                       (idx_t)nq, (const idx_t*)offs, (int)num_types, (idx_t)n, (idx_t)nr, (idx_t)d, q, p, lo, hi, tt, greater, equal, cands,
                       (unsigned long long*)bad);
    HET_LAUNCH_CHECK("HET_rank_prelude");
  }
  if (n == 0) return HET_OK;  // (every query is bad: nothing to rank)
  if (npairs > 0) {
    HET_KTIME("HET_rank_pairs", st);
    hipLaunchKernelGGL(HET_rank_pair_keys, dim3(grid_for(npairs)), dim3(kBlock), 0, st, (const idx_t*)pq, (const idx_t*)pc, (idx_t)npairs, (idx_t)nq,
                       (idx_t)n, (idx_t)nqt, (idx_t)nct, ki, vi);
    HET_LAUNCH_CHECK("HET_rank_pair_keys");
    size_t tb = (size_t)temp;
    HET_HIP(hipcub::DeviceRadixSort::SortPairs(base + L.temp, tb, ki, ko, vi, vo, (int)npairs, 0, bits, st));
    hipLaunchKernelGGL(HET_rank_tile_ptr, dim3(grid_for(nct + 1)), dim3(kBlock), 0, st, (const uint64_t*)ko, (idx_t)npairs, (idx_t)nqt, (idx_t)nct,
                       tile_ptr);
    HET_LAUNCH_CHECK("HET_rank_tile_ptr");
  }
  RankArgs g;
  g.q = q;
  g.p = p;
  g.lo = lo;
  g.hi = hi;
  g.tt = tt;
  g.keys = ko;
  g.vals = vo;
  g.tile_ptr = tile_ptr;
  g.npairs = npairs;
  g.nq = nq;
  g.n = n;
  g.d = d;
  g.nqt = nqt;
  g.nct = nct;
  g.nqc = nqc;
  int64_t span = ceil_div64(nct * nqc, kRankMaxBlocks);
  span = span < 1 ? 1 : (span > kRankMaxSpan ? kRankMaxSpan : span);
  g.span = (int)span;
  g.items = ceil_div64(nct, span) * nqc;
  g.greater = greater;
  g.equal = equal;
  g.cands = cands;
  const unsigned grid = (unsigned)(g.items > kRankMaxBlocks ? kRankMaxBlocks : g.items);
  HET_HIP(hipFuncSetAttribute((const void*)HET_triple_rank<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HET_KTIME("HET_triple_rank", st);
  hipLaunchKernelGGL((HET_triple_rank<T>), dim3(grid), dim3(kBlock), lds, st, h, g);
  HET_LAUNCH_CHECK("HET_triple_rank");
  return HET_OK;
}

}  // namespace

extern "C" int het_triple_rank_params(int64_t* out) {
  HET_REQUIRE(out, "het_triple_rank_params: null pointer");
  out[0] = kRankQueryTile;
  out[1] = kRankCandTile;
  out[2] = kRankMinWidth;
  out[3] = kRankMaxWidth;
  out[4] = kBlock;
  out[5] = kRankMaxBlocks;
  out[6] = kRankChunkTiles;
  out[7] = kRankMaxSpan;
  return HET_OK;
}

extern "C" int64_t het_triple_rank_workspace(int64_t num_queries, int64_t num_pairs, int64_t num_nodes, int64_t dim) {
  const char* op = "het_triple_rank_workspace";
  if (num_queries < 0 || num_queries >= kRankMaxQueries || num_pairs < 0 || num_pairs >= kRankMaxPairs || num_nodes < 0 ||
      num_nodes >= kRankMaxNodes || !rank_width_ok(dim)) {
    het_set_error("%s: num_queries=%lld, num_pairs=%lld, num_nodes=%lld, dim=%lld", op, (long long)num_queries, (long long)num_pairs,
                  (long long)num_nodes, (long long)dim);
    return -1;
  }
  if (num_queries == 0) return 0;
  const int64_t nqt = ceil_div64(num_queries, kRankQueryTile), nct = ceil_div64(num_nodes, kRankCandTile);
  const int64_t temp = rank_temp_bytes(num_pairs, rank_bits((uint64_t)nct * (uint64_t)nqt));
  if (temp < 0) {
    het_set_error("%s: the sort's scratch size could not be asked (no device?)", op);
    return -1;
  }
  return rank_layout(num_queries, num_pairs, num_nodes, dim).temp + temp;
}

extern "C" int het_triple_rank(const float* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth, int64_t num_queries,
                               const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs, const int64_t* node_type_offsets,
                               int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim, int32_t* greater, int32_t* equal,
                               int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes, het_stream stream) {
  return triple_rank("het_triple_rank", false, h, w, anchor, rel, truth, nullptr, num_queries, pair_query, pair_cand, num_pairs,
                     node_type_offsets, num_types, num_nodes, num_rels, dim, greater, equal, cands, bad, workspace, workspace_bytes, stream);
}

extern "C" int het_triple_rank_bf16(const het_bf16* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth,
                                    int64_t num_queries, const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs,
                                    const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim,
                                    int32_t* greater, int32_t* equal, int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes,
                                    het_stream stream) {
  return triple_rank("het_triple_rank_bf16", false, h, w, anchor, rel, truth, nullptr, num_queries, pair_query, pair_cand, num_pairs,
                     node_type_offsets, num_types, num_nodes, num_rels, dim, greater, equal, cands, bad, workspace, workspace_bytes, stream);
}

// ---- ComplEx: the same launches behind its own prelude (side [num_queries]: 0 ranks tails, 1 ranks heads) -----------------------------
extern "C" int het_complex_rank(const float* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth,
                                const int64_t* side, int64_t num_queries, const int64_t* pair_query, const int64_t* pair_cand, int64_t num_pairs,
                                const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t num_rels, int64_t dim,
                                int32_t* greater, int32_t* equal, int32_t* cands, int64_t* bad, void* workspace, int64_t workspace_bytes,
                                het_stream stream) {
  return triple_rank("het_complex_rank", true, h, w, anchor, rel, truth, side, num_queries, pair_query, pair_cand, num_pairs, node_type_offsets,
                     num_types, num_nodes, num_rels, dim, greater, equal, cands, bad, workspace, workspace_bytes, stream);
}

extern "C" int het_complex_rank_bf16(const het_bf16* h, const float* w, const int64_t* anchor, const int64_t* rel, const int64_t* truth,
                                     const int64_t* side, int64_t num_queries, const int64_t* pair_query, const int64_t* pair_cand,
                                     int64_t num_pairs, const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t num_rels,
                                     int64_t dim, int32_t* greater, int32_t* equal, int32_t* cands, int64_t* bad, void* workspace,
                                     int64_t workspace_bytes, het_stream stream) {
  return triple_rank("het_complex_rank_bf16", true, h, w, anchor, rel, truth, side, num_queries, pair_query, pair_cand, num_pairs,
                     node_type_offsets, num_types, num_nodes, num_rels, dim, greater, equal, cands, bad, workspace, workspace_bytes, stream);
}
