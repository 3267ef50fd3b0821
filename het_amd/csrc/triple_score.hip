// Link prediction on triples (s, r, o): keyed corruption of positives, the inverted index of a batch, the DistMult and the ComplEx
// score and their backward (het_amd/linkpred.py; the rules in include/het_amd.h).  One body per kernel: the
// decoder is a type that gives the three per-piece terms (DistMultTerms, ComplExTerms below); the lists, chunks and owners are shared.
//
// The rule (fp32 unless said otherwise; bf16 rows of h are widened first, which is exact):
//   score_j = sum_d h[s_j, d] * w[r_j, d] * h[o_j, d]; a triple with s or o outside [0, N) or r outside [0, R) is BAD: its score is +0,
//   it is in no list of the plan and so in no gradient, and no address is ever formed from such an id.
//   grad_h[v] = the sum over v's slot list, in ascending slot 2j + side, of g_j * w[r_j] (.) h[the other end of triple j]; a list longer
//   than kTripleListChunk slots is cut into chunks of that many from its start, each summed by its own lane group into a partial, and
//   the partials are added in chunk order.  grad_w[r] = the sum over r's triples, in ascending j within chunks of kTripleRelChunk, of
//   g_j * (h[s_j] (.) h[o_j]); the chunk partials are added in chunk order.  Every row of both is written once: +0 where a list is empty.
//
// Lanes: a triple, a node and a chunk each get G = triple_lanes(D) lanes side by side, the power of two with D <= 4 * G, at most
// kTripleMaxLanes; a lane holds pieces of 4 elements (16 bytes of float, 8 of bf16), G pieces apart.  The score adds its G lanes with an
// xor butterfly of cross-lane moves; the gradient passes keep a piece in one lane from the first slot to the store, so nothing crosses
// lanes there.  No LDS.  Every index and row offset is 64-bit.
// The plan is built on the device alone: two stable radix sorts (hipCUB) of 32-bit (id, position) pairs, boundaries by binary search,
// two exclusive scans of the chunk counts.  Nothing is read back and nothing waits for the stream.
//
// ComplEx (the same lists, orders and conventions; D even, column 2k the real and 2k + 1 the imaginary part of component k, so a piece
// is two whole complex numbers and every product stays inside the lane that owns the piece).  With a = h[s_j], b = w[r_j], c = h[o_j]:
//   score_j = sum_k Re(a_k b_k conj(c_k)) = sum_k (a_r b_r - a_i b_i) c_r + (a_r b_i + a_i b_r) c_i
//   slot side 0 (v is the head):  grad a_r += g (b_r c_r + b_i c_i)    grad a_i += g (b_r c_i - b_i c_r)
//   slot side 1 (v is the tail):  grad c_r += g (a_r b_r - a_i b_i)    grad c_i += g (a_r b_i + a_i b_r)
//   grad b_r += g (a_r c_r + a_i c_i)    grad b_i += g (a_r c_i - a_i c_r)
// written as explicit fmaf chains (ComplExTerms), so the roundings are the source's and not the compiler's choice.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "common.hip.h"

namespace {

constexpr int kTripleMinWidth = 4;      // D is a multiple of 4 ...
constexpr int kTripleMaxWidth = 1024;   // ... up to this many columns
constexpr int kTripleMaxLanes = 16;     // a triple gets 1, 2, 4, 8 lanes up to D = 4, 8, 16, 32 and 16 lanes beyond
constexpr int kTripleListChunk = 128;   // L: a node's slot list longer than this is summed in chunks of this many
constexpr int kTripleRelChunk = 256;    // a relation's triples are summed in chunks of this many
constexpr int kTripleMaxBlocks = 16384; // a lane group takes further items beyond this many workgroups
constexpr int64_t kTripleMaxTriples = 1ll << 30, kTripleMaxNodes = 1ll << 31;

int triple_lanes(int64_t d) {
  int g = 1;
  while (g < kTripleMaxLanes && (int64_t)g * 4 < d) g <<= 1;
  return g;
}
bool triple_width_ok(int64_t d) { return d >= kTripleMinWidth && d <= kTripleMaxWidth && d % 4 == 0; }
unsigned triple_blocks(int64_t items, int g) {
  const int64_t b = ceil_div64(items, kBlock / g);
  return (unsigned)(b < 1 ? 1 : (b > kTripleMaxBlocks ? kTripleMaxBlocks : b));
}
// most chunks the long lists of 2t slots can have (a list longer than L has fewer than 2 * len / L), and the relations' t triples
int64_t triple_max_node_chunks(int64_t t) { return 4 * t / kTripleListChunk + 1; }
int64_t triple_max_rel_chunks(int64_t t, int64_t nr) { return t / kTripleRelChunk + nr + 1; }
int triple_bits(int64_t top) {  // bits that hold every value of [0, top]
  int b = 1;
  while (b < 32 && (1ll << b) <= top) ++b;
  return b;
}
int64_t align256(int64_t b) { return (b + 255) & ~255ll; }

#define HET_DISPATCH_TRIPLE_LANES(GV, CALL)         \
  switch (GV) {                                     \
    case 1: { constexpr int G = 1; CALL; break; }   \
    case 2: { constexpr int G = 2; CALL; break; }   \
    case 4: { constexpr int G = 4; CALL; break; }   \
    case 8: { constexpr int G = 8; CALL; break; }   \
    default: { constexpr int G = 16; CALL; break; } \
  }

// ---- keyed corruption: triple j of [0, p * (1 + k)) from the positives; reads no table --------------------------------------------
__global__ __launch_bounds__(kBlock) void HET_triple_corrupt(const idx_t* __restrict__ src, const idx_t* __restrict__ rel,
                                                             const idx_t* __restrict__ dst, idx_t p, idx_t k, uint64_t stream,
                                                             const idx_t* __restrict__ offs, int num_types, idx_t n,
                                                             idx_t* __restrict__ s, idx_t* __restrict__ r, idx_t* __restrict__ o) {
  const idx_t t = p * (1 + k), step = (idx_t)gridDim.x * kBlock;
  for (idx_t j = (idx_t)blockIdx.x * kBlock + threadIdx.x; j < t; j += step) {
    if (j < p) {
      s[j] = src[j];
      r[j] = rel[j];
      o[j] = dst[j];
      continue;
    }
    const idx_t m = j - p, i = m / k;
    const uint64_t key = sm64(stream + (uint64_t)m);
    const bool head = (key >> 63) != 0;
    const uint64_t u = (key >> 31) & 0xFFFFFFFFull;
    const idx_t si = src[i], oi = dst[i];
    const idx_t v_old = head ? si : oi;
    idx_t lo = 0, hi = n;
    bool in = v_old >= 0 && v_old < n;
    if (offs) {
      in = v_old >= offs[0] && v_old < offs[num_types];
      if (in) {
        const int ty = find_segment(offs, num_types, v_old);
        lo = offs[ty];
        hi = offs[ty + 1];
      }
    }
    // (an end outside every run stays what it was: the triple is counted as bad where it is scored)
    const idx_t v_new = in ? lo + (idx_t)((u * (uint64_t)(hi - lo)) >> 32) : v_old;
    s[j] = head ? v_new : si;
    r[j] = rel[i];
    o[j] = head ? oi : v_new;
  }
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// 32-bit sort keys: the node of every slot 2j + side (side 0: the head s_j, side 1: the tail o_j) and the relation of every triple; a
// bad triple gets the key one past the table (N, R), so it sorts behind every list
__global__ __launch_bounds__(kBlock) void HET_triple_keys(const idx_t* __restrict__ s, const idx_t* __restrict__ r, const idx_t* __restrict__ o,
                                                          idx_t t, idx_t n, idx_t nr, uint32_t* __restrict__ nkeys, uint32_t* __restrict__ nvals,
                                                          uint32_t* __restrict__ rkeys, uint32_t* __restrict__ rvals) {
  const idx_t step = (idx_t)gridDim.x * kBlock;
  for (idx_t j = (idx_t)blockIdx.x * kBlock + threadIdx.x; j < t; j += step) {
    const idx_t sj = s[j], rj = r[j], oj = o[j];
    const bool ok = (uint64_t)sj < (uint64_t)n && (uint64_t)oj < (uint64_t)n && (uint64_t)rj < (uint64_t)nr;
    nkeys[2 * j] = (uint32_t)(ok ? sj : n);
    nkeys[2 * j + 1] = (uint32_t)(ok ? oj : n);
    nvals[2 * j] = (uint32_t)(2 * j);
    nvals[2 * j + 1] = (uint32_t)(2 * j + 1);
    rkeys[j] = (uint32_t)(ok ? rj : nr);
    rvals[j] = (uint32_t)j;
  }
}

__device__ __forceinline__ idx_t triple_lower_bound(const uint32_t* __restrict__ a, idx_t len, idx_t key) {
  idx_t lo = 0, hi = len;
  while (lo < hi) {
    const idx_t mid = (lo + hi) >> 1;
    if ((idx_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the sorted positions widened, the boundaries of every list by search, the chunk count of every list, the count of bad triples
__global__ __launch_bounds__(kBlock) void HET_triple_bounds(const uint32_t* __restrict__ nkeys, const uint32_t* __restrict__ nvals,
                                                            const uint32_t* __restrict__ rkeys, const uint32_t* __restrict__ rvals, idx_t t,
                                                            idx_t n, idx_t nr, idx_t* __restrict__ node_ptr, idx_t* __restrict__ node_slots,
                                                            idx_t* __restrict__ rel_ptr, idx_t* __restrict__ rel_order,
                                                            idx_t* __restrict__ counts, idx_t* __restrict__ bad) {
  const idx_t total = 2 * t > n + 1 ? 2 * t : n + 1, all = total > nr + 1 ? total : nr + 1;
  const idx_t step = (idx_t)gridDim.x * kBlock;
  for (idx_t i = (idx_t)blockIdx.x * kBlock + threadIdx.x; i < all; i += step) {
    if (i < 2 * t) node_slots[i] = nvals[i];
    if (i < t) rel_order[i] = rvals[i];
    if (i <= n) {
      const idx_t a = triple_lower_bound(nkeys, 2 * t, i);
      node_ptr[i] = a;
      idx_t c = 0;
      if (i < n) {
        const idx_t len = triple_lower_bound(nkeys, 2 * t, i + 1) - a;
        c = len > kTripleListChunk ? (len + kTripleListChunk - 1) / kTripleListChunk : 0;
      }
      counts[i] = c;
    }
    if (i <= nr) {
      const idx_t a = triple_lower_bound(rkeys, t, i);
      rel_ptr[i] = a;
      idx_t c = 0;
      if (i < nr)
        c = (triple_lower_bound(rkeys, t, i + 1) - a + kTripleRelChunk - 1) / kTripleRelChunk;
      else
        bad[0] = t - a;
      counts[n + 1 + i] = c;
    }
  }
}

// ---- the decoders: the arithmetic of one piece (4 columns) in the score, in a node's walk over its slots and in a relation's walk ----
struct DistMultTerms {
  static constexpr const char* kScore = "HET_distmult_score";
  static constexpr const char* kChunksH = "HET_distmult_grad_chunks_h";
  static constexpr const char* kChunksW = "HET_distmult_grad_chunks_w";
  static constexpr const char* kChunks = "HET_distmult_grad_chunks";
  static constexpr const char* kGradH = "HET_distmult_grad_h";
  static constexpr const char* kGradW = "HET_distmult_grad_w";
  // acc + the piece's four products a * b * c
  static __device__ __forceinline__ float score(float acc, const float4& a, const float4& b, const float4& c) {
    acc += a.x * b.x * c.x;
    acc += a.y * b.y * c.y;
    acc += a.z * b.z * c.z;
    acc += a.w * b.w * c.w;
    return acc;
  }
  // acc += (g * b) * x: b the relation's piece, x the other end's; the side of the slot does not matter
  static __device__ __forceinline__ void slot_term(float4& acc, float gj, const float4& b, const float4& x, bool /*tail*/) {
    acc.x += (gj * b.x) * x.x;
    acc.y += (gj * b.y) * x.y;
    acc.z += (gj * b.z) * x.z;
    acc.w += (gj * b.w) * x.w;
  }
  // acc += (a * c) * g: a the head's piece, c the tail's
  static __device__ __forceinline__ void rel_term(float4& acc, float gj, const float4& a, const float4& c) {
    acc.x += (a.x * c.x) * gj;
    acc.y += (a.y * c.y) * gj;
    acc.z += (a.z * c.z) * gj;
    acc.w += (a.w * c.w) * gj;
  }
};

struct ComplExTerms {
  static constexpr const char* kScore = "HET_complex_score";
  static constexpr const char* kChunksH = "HET_complex_grad_chunks_h";
  static constexpr const char* kChunksW = "HET_complex_grad_chunks_w";
  static constexpr const char* kChunks = "HET_complex_grad_chunks";
  static constexpr const char* kGradH = "HET_complex_grad_h";
  static constexpr const char* kGradW = "HET_complex_grad_w";
  // one complex number: re = a_r b_r - a_i b_i, im = a_r b_i + a_i b_r, then acc = fmaf(im, c_i, fmaf(re, c_r, acc))
  static __device__ __forceinline__ float score1(float acc, float ar, float ai, float br, float bi, float cr, float ci) {
    const float re = fmaf(-ai, bi, ar * br), im = fmaf(ai, br, ar * bi);
    return fmaf(im, ci, fmaf(re, cr, acc));
  }
  static __device__ __forceinline__ float score(float acc, const float4& a, const float4& b, const float4& c) {
    acc = score1(acc, a.x, a.y, b.x, b.y, c.x, c.y);
    return score1(acc, a.z, a.w, b.z, b.w, c.z, c.w);
  }
  // one complex number with u = g b_r, v = g b_i negated on a tail slot:  re += u x_r + v x_i,  im += u x_i - v x_r
  // (head slot, x = c: g (b_r c_r + b_i c_i), g (b_r c_i - b_i c_r); tail slot, x = a: g (a_r b_r - a_i b_i), g (a_r b_i + a_i b_r))
  static __device__ __forceinline__ void slot1(float& re, float& im, float u, float v, float xr, float xi) {
    re = fmaf(v, xi, fmaf(u, xr, re));
    im = fmaf(-v, xr, fmaf(u, xi, im));
  }
  static __device__ __forceinline__ void slot_term(float4& acc, float gj, const float4& b, const float4& x, bool tail) {
    const float u0 = gj * b.x, v0 = gj * b.y, u1 = gj * b.z, v1 = gj * b.w;
    slot1(acc.x, acc.y, u0, tail ? -v0 : v0, x.x, x.y);
    slot1(acc.z, acc.w, u1, tail ? -v1 : v1, x.z, x.w);
  }
  // one complex number: re += (a_r c_r + a_i c_i) g,  im += (a_r c_i - a_i c_r) g
  static __device__ __forceinline__ void rel1(float& re, float& im, float gj, float ar, float ai, float cr, float ci) {
    re = fmaf(fmaf(ai, ci, ar * cr), gj, re);
    im = fmaf(fmaf(-ai, cr, ar * ci), gj, im);
  }
  static __device__ __forceinline__ void rel_term(float4& acc, float gj, const float4& a, const float4& c) {
    rel1(acc.x, acc.y, gj, a.x, a.y, c.x, c.y);
    rel1(acc.z, acc.w, gj, a.z, a.w, c.z, c.w);
  }
};

// ---- the score ---------------------------------------------------------------------------------------------------------------------
template <typename DEC, typename T, int G>
__global__ __launch_bounds__(kBlock) void HET_triple_score(const T* __restrict__ h, const float* __restrict__ w, const idx_t* __restrict__ s,
                                                           const idx_t* __restrict__ r, const idx_t* __restrict__ o, idx_t t, idx_t n, idx_t nr,
                                                           idx_t d, float* __restrict__ score) {
  constexpr int GPB = kBlock / G;
  const int gi = threadIdx.x / G, l = threadIdx.x % G;
  const idx_t step = (idx_t)gridDim.x * GPB, np = d >> 2;
  for (idx_t j0 = (idx_t)blockIdx.x * GPB; j0 < t; j0 += step) {  // (the same trip count in every lane of a wave: the butterfly below)
    const idx_t j = j0 + gi;
    const bool in = j < t;
    idx_t sj = -1, rj = -1, oj = -1;
    if (in) {
      sj = s[j];
      rj = r[j];
      oj = o[j];
    }
    const bool ok = (uint64_t)sj < (uint64_t)n && (uint64_t)oj < (uint64_t)n && (uint64_t)rj < (uint64_t)nr;
    float acc = 0.f;
    if (ok) {
      const T* hs = h + sj * d;
      const T* ho = h + oj * d;
      const float* wr = w + rj * d;
      for (idx_t p = l; p < np; p += G) {
        const float4 a = ldrow4(hs + 4 * p), b = ld4(wr + 4 * p), c = ldrow4(ho + 4 * p);
        acc = DEC::score(acc, a, b, c);
      }
    }
#pragma unroll
    for (int x = G / 2; x > 0; x >>= 1) acc += __shfl_xor(acc, x);
    if (in && l == 0) score[j] = acc;
  }
}

// ---- the backward ------------------------------------------------------------------------------------------------------------------
struct TripleIds {
  const idx_t* s;
  const idx_t* r;
  const idx_t* o;
  idx_t t, n, nr, d;
};

// piece p of sum over the slots at positions [b, e) of the decoder's slot term (DistMult: g_j * w[r_j] (.) h[other end]), in that
// order.  An id is used as an index only when it lies inside its table (the plan lists no other; a plan that is not this batch's
// reads nothing out of bounds either).
template <typename DEC, typename T>
__device__ __forceinline__ float4 triple_sum_slots(const T* __restrict__ h, const float* __restrict__ w, const float* __restrict__ g,
                                                   const TripleIds& ids, const idx_t* __restrict__ slots, idx_t b, idx_t e, idx_t p) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (idx_t pos = b; pos < e; ++pos) {
    const idx_t slot = slots[pos], j = slot >> 1;
    if ((uint64_t)j >= (uint64_t)ids.t) continue;
    const idx_t other = (slot & 1) ? ids.s[j] : ids.o[j], rj = ids.r[j];
    if ((uint64_t)other >= (uint64_t)ids.n || (uint64_t)rj >= (uint64_t)ids.nr) continue;
    const float gj = g[j];
    const float4 a = ld4(w + rj * ids.d + 4 * p), c = ldrow4(h + other * ids.d + 4 * p);
    DEC::slot_term(acc, gj, a, c, (slot & 1) != 0);
  }
  return acc;
}

// piece p of the sum over the triples at positions [b, e) of a relation's order of the decoder's relation term (DistMult:
// g_j * (h[s_j] (.) h[o_j])), in that order
template <typename DEC, typename T>
__device__ __forceinline__ float4 triple_sum_rel(const T* __restrict__ h, const float* __restrict__ g, const TripleIds& ids,
                                                 const idx_t* __restrict__ order, idx_t b, idx_t e, idx_t p) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (idx_t pos = b; pos < e; ++pos) {
    const idx_t j = order[pos];
    if ((uint64_t)j >= (uint64_t)ids.t) continue;
    const idx_t sj = ids.s[j], oj = ids.o[j];
    if ((uint64_t)sj >= (uint64_t)ids.n || (uint64_t)oj >= (uint64_t)ids.n) continue;
    const float gj = g[j];
    const float4 a = ldrow4(h + sj * ids.d + 4 * p), c = ldrow4(h + oj * ids.d + 4 * p);
    DEC::rel_term(acc, gj, a, c);
  }
  return acc;
}

// the list that owns chunk c: the last i of [0, lists) with cptr[i] <= c (lists without chunks repeat their neighbour's value)
__device__ __forceinline__ idx_t triple_chunk_owner(const idx_t* __restrict__ cptr, idx_t lists, idx_t c) {
  idx_t lo = 0, hi = lists;
  while (hi - lo > 1) {
    const idx_t mid = (lo + hi) >> 1;
    if (cptr[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ idx_t triple_clamp(idx_t v, idx_t top) { return v < 0 ? 0 : (v > top ? top : v); }

// one lane group per chunk of a list: `lists` lists with boundaries ptr and chunk offsets cptr, chunks of `chunk` positions.
// REL: the lists are relations (grad_w), else nodes (grad_h).  part [max_chunks, d] floats.
template <typename DEC, typename T, int G, bool REL>
__global__ __launch_bounds__(kBlock) void HET_triple_grad_chunks(const T* __restrict__ h, const float* __restrict__ w, const float* __restrict__ g,
                                                                  TripleIds ids, const idx_t* __restrict__ ptr, const idx_t* __restrict__ list,
                                                                  const idx_t* __restrict__ cptr, idx_t lists, idx_t chunk, idx_t positions,
                                                                  idx_t max_chunks, float* __restrict__ part) {
  constexpr int GPB = kBlock / G;
  const int gi = threadIdx.x / G, l = threadIdx.x % G;
  const idx_t step = (idx_t)gridDim.x * GPB, np = ids.d >> 2;
  idx_t total = cptr[lists];
  if (total > max_chunks) total = max_chunks;
  for (idx_t c = (idx_t)blockIdx.x * GPB + gi; c < total; c += step) {
    const idx_t v = triple_chunk_owner(cptr, lists, c);
    const idx_t end = triple_clamp(ptr[v + 1], positions);
    const idx_t b = triple_clamp(ptr[v] + (c - cptr[v]) * chunk, end);
    const idx_t e = b + chunk < end ? b + chunk : end;
    for (idx_t p = l; p < np; p += G) {
      const float4 acc = REL ? triple_sum_rel<DEC>(h, g, ids, list, b, e, p) : triple_sum_slots<DEC>(h, w, g, ids, list, b, e, p);
      st4(part + c * ids.d + 4 * p, acc);
    }
  }
}

// one lane group per node: a list of at most L slots summed here, a longer one from its chunk partials in chunk order; every row stored
template <typename DEC, typename T, int G>
__global__ __launch_bounds__(kBlock) void HET_triple_grad_h(const T* __restrict__ h, const float* __restrict__ w, const float* __restrict__ g,
                                                             TripleIds ids, const idx_t* __restrict__ node_ptr, const idx_t* __restrict__ slots,
                                                             const idx_t* __restrict__ cptr, idx_t max_chunks, const float* __restrict__ part,
                                                             T* __restrict__ gh) {
  constexpr int GPB = kBlock / G;
  const int gi = threadIdx.x / G, l = threadIdx.x % G;
  const idx_t step = (idx_t)gridDim.x * GPB, np = ids.d >> 2, positions = 2 * ids.t;
  for (idx_t v = (idx_t)blockIdx.x * GPB + gi; v < ids.n; v += step) {
    idx_t b = 0, e = 0;
    if (ids.t > 0) {  // (no triples: no plan to read)
      e = triple_clamp(node_ptr[v + 1], positions);
      b = triple_clamp(node_ptr[v], e);
    }
    const bool chunked = e - b > kTripleListChunk;
    idx_t c0 = 0, c1 = 0;
    if (chunked) {
      c1 = triple_clamp(cptr[v + 1], max_chunks);
      c0 = triple_clamp(cptr[v], c1);
    }
    for (idx_t p = l; p < np; p += G) {
      float4 acc;
      if (chunked) {
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (idx_t c = c0; c < c1; ++c) {
          const float4 q = ld4(part + c * ids.d + 4 * p);
          acc.x += q.x;
          acc.y += q.y;
          acc.z += q.z;
          acc.w += q.w;
        }
      } else {
        acc = triple_sum_slots<DEC>(h, w, g, ids, slots, b, e, p);
      }
      strow4(gh + v * ids.d + 4 * p, acc);
    }
  }
}

// one lane group per relation: its chunk partials in chunk order (the same for every decoder)
template <int G>
__global__ __launch_bounds__(kBlock) void HET_triple_grad_w(const idx_t* __restrict__ cptr, idx_t t, idx_t nr, idx_t d, idx_t max_chunks,
                                                             const float* __restrict__ part, float* __restrict__ gw) {
  constexpr int GPB = kBlock / G;
  const int gi = threadIdx.x / G, l = threadIdx.x % G;
  const idx_t step = (idx_t)gridDim.x * GPB, np = d >> 2;
  for (idx_t rel = (idx_t)blockIdx.x * GPB + gi; rel < nr; rel += step) {
    idx_t c0 = 0, c1 = 0;
    if (t > 0) {
      c1 = triple_clamp(cptr[rel + 1], max_chunks);
      c0 = triple_clamp(cptr[rel], c1);
    }
    for (idx_t p = l; p < np; p += G) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (idx_t c = c0; c < c1; ++c) {
        const float4 q = ld4(part + c * d + 4 * p);
        acc.x += q.x;
        acc.y += q.y;
        acc.z += q.z;
        acc.w += q.w;
      }
      st4(gw + rel * d + 4 * p, acc);
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
int triple_check_sizes(const char* op, int64_t t, int64_t n, int64_t nr) {
  HET_REQUIRE(t >= 0 && t < kTripleMaxTriples, "%s: num_triples=%lld (0 <= num_triples < 2^30)", op, (long long)t);
  HET_REQUIRE(n >= 0 && n < kTripleMaxNodes, "%s: num_nodes=%lld (0 <= num_nodes < 2^31)", op, (long long)n);
  HET_REQUIRE(nr >= 0 && nr < kTripleMaxNodes, "%s: num_rels=%lld (0 <= num_rels < 2^31)", op, (long long)nr);
  return HET_OK;
}

int triple_check_width(const char* op, int64_t d) {
  HET_REQUIRE(d >= 1, "%s: dim=%lld (at least one column)", op, (long long)d);
  if (!triple_width_ok(d)) {
    het_set_error("%s: dim=%lld is not a width the kernels take (a multiple of 4 from %d to %d)", op, (long long)d, kTripleMinWidth,
                  kTripleMaxWidth);
    return HET_ERR_UNSUPPORTED;
  }
  return HET_OK;
}

// the fixed part of the plan's workspace: the sort keys and positions in and out, the chunk counts
struct PlanLayout {
  int64_t nkeys_in, nkeys_out, nvals_in, nvals_out, rkeys_in, rkeys_out, rvals_in, rvals_out, counts, temp;
};
PlanLayout plan_layout(int64_t t, int64_t n, int64_t nr) {
  PlanLayout L;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t here = at; at += align256(bytes); return here; };
  L.nkeys_in = take(8 * t);
  L.nkeys_out = take(8 * t);
  L.nvals_in = take(8 * t);
  L.nvals_out = take(8 * t);
  L.rkeys_in = take(4 * t);
  L.rkeys_out = take(4 * t);
  L.rvals_in = take(4 * t);
  L.rvals_out = take(4 * t);
  L.counts = take(8 * (n + nr + 2));
  L.temp = at;
  return L;
}

// bytes of hipCUB's own scratch for the plan's two sorts and two scans (the largest of the four); a negative HET_ERR code on failure
int64_t plan_temp_bytes(int64_t t, int64_t n, int64_t nr) {
  size_t a = 0, b = 0, c = 0, d = 0;
  uint32_t* k = nullptr;
  idx_t* q = nullptr;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, k, k, k, (int)(2 * t), 0, triple_bits(n), (hipStream_t)0) != hipSuccess ||
      hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, k, k, k, (int)t, 0, triple_bits(nr), (hipStream_t)0) != hipSuccess ||
      hipcub::DeviceScan::ExclusiveSum(nullptr, c, q, q, (int)(n + 1), (hipStream_t)0) != hipSuccess ||
      hipcub::DeviceScan::ExclusiveSum(nullptr, d, q, q, (int)(nr + 1), (hipStream_t)0) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  const size_t m = std::max(std::max(a, b), std::max(c, d));
  return align256((int64_t)m);
}

template <typename DEC, typename T>
int triple_score(const char* op, const T* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t t, int64_t n,
                   int64_t nr, int64_t d, float* score, het_stream stream) {
  int rc = triple_check_sizes(op, t, n, nr);
  if (rc != HET_OK) return rc;
  rc = triple_check_width(op, d);
  if (rc != HET_OK) return rc;
  if (t == 0) return HET_OK;
  HET_REQUIRE(s && r && o && score && (h || n == 0) && (w || nr == 0), "%s: null pointer", op);
  HET_REQUIRE((sizeof(T) == 4 ? aligned16(h) : aligned8(h)) && aligned16(w) && aligned8(s, r, o) && ((uintptr_t)score & 3) == 0,
              "%s: misaligned pointer (h on %d-byte, w on 16-byte, ids on 8-byte, score on 4-byte boundaries)", op, (int)(4 * sizeof(T)));
  const int g = triple_lanes(d);
  hipStream_t st = (hipStream_t)stream;
  HET_KTIME(DEC::kScore, st);
  HET_DISPATCH_TRIPLE_LANES(g, hipLaunchKernelGGL((HET_triple_score<DEC, T, G>), dim3(triple_blocks(t, g)), dim3(kBlock), 0, st, h, w, (const idx_t*)s,
                                                  (const idx_t*)r, (const idx_t*)o, (idx_t)t, (idx_t)n, (idx_t)nr, (idx_t)d, score));
  HET_LAUNCH_CHECK(DEC::kScore);
  return HET_OK;
}

int64_t backward_workspace_bytes(int64_t t, int64_t nr, int64_t d) {
  return t == 0 ? 0 : (triple_max_node_chunks(t) + triple_max_rel_chunks(t, nr)) * d * 4;
}

template <typename DEC, typename T>
int triple_score_backward(const char* op, const T* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                            const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                            const int64_t* rel_order, const int64_t* chunk_ptr, int64_t t, int64_t n, int64_t nr, int64_t d, T* grad_h,
                            float* grad_w, void* workspace, int64_t workspace_bytes, het_stream stream) {
  int rc = triple_check_sizes(op, t, n, nr);
  if (rc != HET_OK) return rc;
  rc = triple_check_width(op, d);
  if (rc != HET_OK) return rc;
  if (t > 0) {
    HET_REQUIRE(s && r && o && grad_score && node_ptr && node_slots && rel_ptr && rel_order && chunk_ptr && (h || n == 0) && (w || nr == 0),
                "%s: null pointer", op);
  }
  HET_REQUIRE((sizeof(T) == 4 ? aligned16(h, grad_h) : aligned8(h, grad_h)) && aligned16(w, grad_w, workspace) &&
                  aligned8(s, r, o, node_ptr, node_slots, rel_ptr, rel_order, chunk_ptr) && ((uintptr_t)grad_score & 3) == 0,
              "%s: misaligned pointer (h and grad_h on %d-byte, w, grad_w and workspace on 16-byte, ids and plan on 8-byte, grad_score on 4-byte "
              "boundaries)", op, (int)(4 * sizeof(T)));
  const int64_t need = backward_workspace_bytes(t, nr, d);
  HET_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace of %lld bytes, %lld needed (het_distmult_score_backward_workspace)",
              op, (long long)(workspace ? workspace_bytes : 0), (long long)need);
  if (h && grad_h) {
    const uintptr_t a = (uintptr_t)h, b = (uintptr_t)grad_h, bytes = (uintptr_t)n * (uintptr_t)d * sizeof(T);
    HET_REQUIRE(!(a < b + bytes && b < a + bytes), "%s: grad_h overlaps h (not an in-place operation)", op);
  }
  hipStream_t st = (hipStream_t)stream;
  const int g = triple_lanes(d);
  const TripleIds ids{(const idx_t*)s, (const idx_t*)r, (const idx_t*)o, (idx_t)t, (idx_t)n, (idx_t)nr, (idx_t)d};
  const int64_t node_chunks = triple_max_node_chunks(t), rel_chunks = triple_max_rel_chunks(t, nr);
  float* part_h = (float*)workspace;
  float* part_w = part_h ? part_h + node_chunks * d : nullptr;
  const idx_t* ncp = (const idx_t*)chunk_ptr;
  const idx_t* rcp = ncp ? ncp + n + 1 : nullptr;
  if (grad_h && n > 0) {
    if (t > 0) {
      HET_KTIME(DEC::kChunksH, st);
      HET_DISPATCH_TRIPLE_LANES(g, hipLaunchKernelGGL((HET_triple_grad_chunks<DEC, T, G, false>), dim3(triple_blocks(node_chunks, g)), dim3(kBlock), 0, st,
                                                      h, w, grad_score, ids, (const idx_t*)node_ptr, (const idx_t*)node_slots, ncp, (idx_t)n,
                                                      (idx_t)kTripleListChunk, (idx_t)(2 * t), (idx_t)node_chunks, part_h));
      HET_LAUNCH_CHECK(DEC::kChunks);
    }
    HET_KTIME(DEC::kGradH, st);
    HET_DISPATCH_TRIPLE_LANES(g, hipLaunchKernelGGL((HET_triple_grad_h<DEC, T, G>), dim3(triple_blocks(n, g)), dim3(kBlock), 0, st, h, w, grad_score, ids,
                                                    (const idx_t*)node_ptr, (const idx_t*)node_slots, ncp, (idx_t)node_chunks,
                                                    (const float*)part_h, grad_h));
    HET_LAUNCH_CHECK(DEC::kGradH);
  }
  if (grad_w && nr > 0) {
    if (t > 0) {
      HET_KTIME(DEC::kChunksW, st);
      HET_DISPATCH_TRIPLE_LANES(g, hipLaunchKernelGGL((HET_triple_grad_chunks<DEC, T, G, true>), dim3(triple_blocks(rel_chunks, g)), dim3(kBlock), 0, st,
                                                      h, w, grad_score, ids, (const idx_t*)rel_ptr, (const idx_t*)rel_order, rcp, (idx_t)nr,
                                                      (idx_t)kTripleRelChunk, (idx_t)t, (idx_t)rel_chunks, part_w));
      HET_LAUNCH_CHECK(DEC::kChunks);
    }
    HET_KTIME(DEC::kGradW, st);
    HET_DISPATCH_TRIPLE_LANES(g, hipLaunchKernelGGL((HET_triple_grad_w<G>), dim3(triple_blocks(nr, g)), dim3(kBlock), 0, st, rcp, (idx_t)t, (idx_t)nr,
                                                    (idx_t)d, (idx_t)rel_chunks, (const float*)part_w, grad_w));
    HET_LAUNCH_CHECK(DEC::kGradW);
  }
  return HET_OK;
}

}  // namespace

extern "C" int het_triple_params(int64_t* out) {
  HET_REQUIRE(out, "het_triple_params: null pointer");
  out[0] = kTripleMinWidth;
  out[1] = kTripleMaxWidth;
  out[2] = kTripleMaxLanes;
  out[3] = kTripleListChunk;
  out[4] = kTripleRelChunk;
  out[5] = kTripleMaxBlocks;
  out[6] = kBlock;
  return HET_OK;
}

extern "C" int het_triple_corrupt(const int64_t* src, const int64_t* rel, const int64_t* dst, int64_t num_pos, int64_t num_neg, int64_t seed,
                                  int64_t draw, const int64_t* node_type_offsets, int64_t num_types, int64_t num_nodes, int64_t* s, int64_t* r,
                                  int64_t* o, het_stream stream) {
  const char* op = "het_triple_corrupt";
  HET_REQUIRE(num_pos >= 0 && num_neg >= 0, "%s: num_pos=%lld, num_neg=%lld", op, (long long)num_pos, (long long)num_neg);
  HET_REQUIRE(num_nodes >= 0 && num_nodes < kTripleMaxNodes, "%s: num_nodes=%lld (0 <= num_nodes < 2^31)", op, (long long)num_nodes);
  HET_REQUIRE(num_types >= 0 && num_types < kTripleMaxNodes, "%s: num_types=%lld", op, (long long)num_types);
  HET_REQUIRE(num_neg < kTripleMaxTriples && num_pos * (1 + num_neg) < kTripleMaxTriples, "%s: num_pos=%lld with num_neg=%lld is 2^30 triples or more", op,
              (long long)num_pos, (long long)num_neg);
  HET_REQUIRE(!node_type_offsets || num_types >= 1, "%s: node_type_offsets with num_types=%lld", op, (long long)num_types);
  if (num_pos == 0) return HET_OK;
  HET_REQUIRE(src && rel && dst && s && r && o, "%s: null pointer", op);
  HET_REQUIRE(aligned8(src, rel, dst, s, r, o, node_type_offsets), "%s: misaligned pointer (int64 arrays on 8-byte boundaries)", op);
  const uint64_t stream_key = sm64((uint64_t)seed ^ sm64((uint64_t)draw));
  hipStream_t st = (hipStream_t)stream;
  HET_KTIME("HET_triple_corrupt", st);
  hipLaunchKernelGGL(HET_triple_corrupt, dim3(grid_for(num_pos * (1 + num_neg))), dim3(kBlock), 0, st, (const idx_t*)src, (const idx_t*)rel,
                     (const idx_t*)dst, (idx_t)num_pos, (idx_t)num_neg, stream_key, (const idx_t*)(node_type_offsets), (int)num_types,
                     (idx_t)num_nodes, (idx_t*)s, (idx_t*)r, (idx_t*)o);
  HET_LAUNCH_CHECK("HET_triple_corrupt");
  return HET_OK;
}

extern "C" int64_t het_triple_plan_workspace(int64_t num_triples, int64_t num_nodes, int64_t num_rels) {
  const char* op = "het_triple_plan_workspace";
  if (num_triples < 0 || num_triples >= kTripleMaxTriples || num_nodes < 0 || num_nodes >= kTripleMaxNodes - 1 || num_rels < 0 ||
      num_rels >= kTripleMaxNodes - 1) {
    het_set_error("%s: num_triples=%lld, num_nodes=%lld, num_rels=%lld", op, (long long)num_triples, (long long)num_nodes, (long long)num_rels);
    return -1;
  }
  if (num_triples == 0) return 0;
  const int64_t temp = plan_temp_bytes(num_triples, num_nodes, num_rels);
  if (temp < 0) {
    het_set_error("%s: the sort's scratch size could not be asked (no device?)", op);
    return -1;
  }
  return plan_layout(num_triples, num_nodes, num_rels).temp + temp;
}

extern "C" int het_triple_plan(const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples, int64_t num_nodes, int64_t num_rels,
                               int64_t* node_ptr, int64_t* node_slots, int64_t* rel_ptr, int64_t* rel_order, int64_t* chunk_ptr, int64_t* bad,
                               void* workspace, int64_t workspace_bytes, het_stream stream) {
  const char* op = "het_triple_plan";
  const int64_t t = num_triples, n = num_nodes, nr = num_rels;
  const int rc = triple_check_sizes(op, t, n, nr);
  if (rc != HET_OK) return rc;
  HET_REQUIRE(n < kTripleMaxNodes - 1 && nr < kTripleMaxNodes - 1, "%s: num_nodes=%lld, num_rels=%lld (below 2^31 - 1)", op, (long long)n, (long long)nr);
  if (t == 0) return HET_OK;
  HET_REQUIRE(s && r && o && node_ptr && node_slots && rel_ptr && rel_order && chunk_ptr && bad, "%s: null pointer", op);
  HET_REQUIRE(aligned8(s, r, o, node_ptr, node_slots, rel_ptr, rel_order, chunk_ptr, bad) && aligned16(workspace),
              "%s: misaligned pointer (int64 arrays on 8-byte, workspace on 16-byte boundaries)", op);
  const PlanLayout L = plan_layout(t, n, nr);
  HET_REQUIRE(workspace && workspace_bytes >= L.temp, "%s: workspace of %lld bytes, more than %lld needed (het_triple_plan_workspace)", op,
              (long long)(workspace ? workspace_bytes : 0), (long long)L.temp);
  const int64_t temp = plan_temp_bytes(t, n, nr);
  if (temp < 0) {
    het_set_error("%s: the sort's scratch size could not be asked", op);
    return HET_ERR_HIP;
  }
  HET_REQUIRE(workspace_bytes >= L.temp + temp, "%s: workspace of %lld bytes, %lld needed (het_triple_plan_workspace)", op,
              (long long)workspace_bytes, (long long)(L.temp + temp));
  char* base = (char*)workspace;
  uint32_t *nki = (uint32_t*)(base + L.nkeys_in), *nko = (uint32_t*)(base + L.nkeys_out), *nvi = (uint32_t*)(base + L.nvals_in),
           *nvo = (uint32_t*)(base + L.nvals_out), *rki = (uint32_t*)(base + L.rkeys_in), *rko = (uint32_t*)(base + L.rkeys_out),
           *rvi = (uint32_t*)(base + L.rvals_in), *rvo = (uint32_t*)(base + L.rvals_out);
  idx_t* counts = (idx_t*)(base + L.counts);
  void* tmp = base + L.temp;
  size_t tb = (size_t)temp;
  hipStream_t st = (hipStream_t)stream;
  HET_KTIME("HET_triple_plan", st);
  hipLaunchKernelGGL(HET_triple_keys, dim3(grid_for(t)), dim3(kBlock), 0, st, (const idx_t*)s, (const idx_t*)r, (const idx_t*)o, (idx_t)t, (idx_t)n,
                     (idx_t)nr, nki, nvi, rki, rvi);
  HET_LAUNCH_CHECK("HET_triple_keys");
  HET_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, nki, nko, nvi, nvo, (int)(2 * t), 0, triple_bits(n), st));
  tb = (size_t)temp;
  HET_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, rki, rko, rvi, rvo, (int)t, 0, triple_bits(nr), st));
  const int64_t all = std::max(std::max(2 * t, n + 1), nr + 1);
  hipLaunchKernelGGL(HET_triple_bounds, dim3(grid_for(all)), dim3(kBlock), 0, st, (const uint32_t*)nko, (const uint32_t*)nvo, (const uint32_t*)rko,
                     (const uint32_t*)rvo, (idx_t)t, (idx_t)n, (idx_t)nr, (idx_t*)node_ptr, (idx_t*)node_slots, (idx_t*)rel_ptr, (idx_t*)rel_order,
                     counts, (idx_t*)bad);
  HET_LAUNCH_CHECK("HET_triple_bounds");
  tb = (size_t)temp;
  HET_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, counts, (idx_t*)chunk_ptr, (int)(n + 1), st));
  tb = (size_t)temp;
  HET_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, counts + n + 1, (idx_t*)chunk_ptr + n + 1, (int)(nr + 1), st));
  return HET_OK;
}

extern "C" int het_distmult_score(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                                  int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream) {
  return triple_score<DistMultTerms>("het_distmult_score", h, w, s, r, o, num_triples, num_nodes, num_rels, dim, score, stream);
}

extern "C" int het_distmult_score_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                                       int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream) {
  return triple_score<DistMultTerms>("het_distmult_score_bf16", h, w, s, r, o, num_triples, num_nodes, num_rels, dim, score, stream);
}

extern "C" int64_t het_distmult_score_backward_workspace(int64_t num_triples, int64_t num_rels, int64_t dim) {
  if (num_triples < 0 || num_triples >= kTripleMaxTriples || num_rels < 0 || num_rels >= kTripleMaxNodes || !triple_width_ok(dim)) {
    het_set_error("het_distmult_score_backward_workspace: num_triples=%lld, num_rels=%lld, dim=%lld", (long long)num_triples, (long long)num_rels,
                  (long long)dim);
    return -1;
  }
  return backward_workspace_bytes(num_triples, num_rels, dim);
}

extern "C" int het_distmult_score_backward(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                           const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                                           const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples, int64_t num_nodes,
                                           int64_t num_rels, int64_t dim, float* grad_h, float* grad_w, void* workspace, int64_t workspace_bytes,
                                           het_stream stream) {
  return triple_score_backward<DistMultTerms>("het_distmult_score_backward", h, w, s, r, o, grad_score, node_ptr, node_slots, rel_ptr, rel_order, chunk_ptr,
                                 num_triples, num_nodes, num_rels, dim, grad_h, grad_w, workspace, workspace_bytes, stream);
}

extern "C" int het_distmult_score_backward_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                                const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots,
                                                const int64_t* rel_ptr, const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples,
                                                int64_t num_nodes, int64_t num_rels, int64_t dim, het_bf16* grad_h, float* grad_w, void* workspace,
                                                int64_t workspace_bytes, het_stream stream) {
  return triple_score_backward<DistMultTerms>("het_distmult_score_backward_bf16", h, w, s, r, o, grad_score, node_ptr, node_slots, rel_ptr, rel_order, chunk_ptr,
                                 num_triples, num_nodes, num_rels, dim, grad_h, grad_w, workspace, workspace_bytes, stream);
}

// ---- ComplEx: the same entries over the same plan and workspace (dim a multiple of 4: whole complex numbers in every piece) ----------
extern "C" int het_complex_score(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                                 int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream) {
  return triple_score<ComplExTerms>("het_complex_score", h, w, s, r, o, num_triples, num_nodes, num_rels, dim, score, stream);
}

extern "C" int het_complex_score_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o, int64_t num_triples,
                                      int64_t num_nodes, int64_t num_rels, int64_t dim, float* score, het_stream stream) {
  return triple_score<ComplExTerms>("het_complex_score_bf16", h, w, s, r, o, num_triples, num_nodes, num_rels, dim, score, stream);
}

extern "C" int het_complex_score_backward(const float* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                          const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots, const int64_t* rel_ptr,
                                          const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples, int64_t num_nodes,
                                          int64_t num_rels, int64_t dim, float* grad_h, float* grad_w, void* workspace, int64_t workspace_bytes,
                                          het_stream stream) {
  return triple_score_backward<ComplExTerms>("het_complex_score_backward", h, w, s, r, o, grad_score, node_ptr, node_slots, rel_ptr, rel_order,
                                             chunk_ptr, num_triples, num_nodes, num_rels, dim, grad_h, grad_w, workspace, workspace_bytes, stream);
}

extern "C" int het_complex_score_backward_bf16(const het_bf16* h, const float* w, const int64_t* s, const int64_t* r, const int64_t* o,
                                               const float* grad_score, const int64_t* node_ptr, const int64_t* node_slots,
                                               const int64_t* rel_ptr, const int64_t* rel_order, const int64_t* chunk_ptr, int64_t num_triples,
                                               int64_t num_nodes, int64_t num_rels, int64_t dim, het_bf16* grad_h, float* grad_w, void* workspace,
                                               int64_t workspace_bytes, het_stream stream) {
  return triple_score_backward<ComplExTerms>("het_complex_score_backward_bf16", h, w, s, r, o, grad_score, node_ptr, node_slots, rel_ptr, rel_order,
                                             chunk_ptr, num_triples, num_nodes, num_rels, dim, grad_h, grad_w, workspace, workspace_bytes, stream);
}
