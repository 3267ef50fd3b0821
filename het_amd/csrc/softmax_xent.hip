// Softmax cross-entropy over the rows of [N, C] logits with integer labels: the forward as one streaming pass plus a one-wave finish,
// the backward as one streaming pass (het_amd/layers.py SoftmaxCrossEntropy; the rule in include/het_amd.h).
//
// The rule (fp32 unless said otherwise; bf16 logits are widened first, which is exact):
//   row i is valid when labels[i] != ignore_index and 0 <= labels[i] < C; any other row is skipped, and counted as bad when its label
//   is not ignore_index.  No address is ever formed from a label that has not passed that test.
//   m = max_c z_c    lse = m + logf(sum_c exp(z_c - m))    loss_i = logf(sum) + (m - z[label])      (lse NaN for a row of -inf, a NaN, +inf)
//   correct_i = z[label] is the first of the row's maxima, a NaN ordered above everything (torch.argmax on the CPU)
//   loss = sum_i loss_i ("sum") or that / valid ("mean"): every wave sums its rows in fp64 in a fixed order and stores one partial;
//   one wave adds the partials in a fixed order.  The three counters take the same road, so nothing is an atomic and nothing is
//   zero-filled first.
//   grad[i, c] = (exp(z_c - lse_i) - [c == label_i]) * g * (1 | 1 / valid), g and valid read from device memory; +0 for a skipped row.
//
// Lanes and rows: a row of C columns gets G = xent_lanes(C) lanes, the power of two with C <= G * kXentLaneElems, at most a wave
// (kXentMaxLanes): 64 / G rows per wave, the lanes of a row side by side.  A lane strides over its row in pieces of 4 columns (16
// bytes of float, 8 of bf16).  A row whose first element is not on such a boundary (C % 4 != 0: C = 3 floats have a 12-byte stride)
// starts with up to 3 single elements, so that the pieces of every row are aligned whatever C is; up to 3 single elements end it.
// Reductions inside the G lanes and inside the wave are xor butterflies of cross-lane moves.  No LDS.  Every index is 64-bit.
// The forward streams an ordinary row once with a short instruction sequence per logit (xent_take) and scans a row that holds a NaN
// or +inf, or nothing but -inf, a second time with the careful one (xent_take_careful); which of the two a row gets depends on its
// own logits only.
#include <float.h>
#include <math.h>

#include "common.hip.h"

namespace {

constexpr int kXentLaneElems = 32;       // a row gets a second lane from C > 32 on, a third and fourth from C > 64 on, ...
constexpr int kXentMaxLanes = HET_WAVE;  // ... and a whole wave from C > kXentLaneElems * kXentMaxLanes / 2 = 1024 on
constexpr int kXentMaxBlocks = 2048;     // 8 workgroups per CU of a 256-CU part; a wave takes further rows beyond kXentMaxBlocks * kBlock / G
constexpr int kXentWavesPerBlock = kBlock / HET_WAVE;
constexpr int kXentPartialBytes = 32;    // per wave: the fp64 loss partial and three int64 counters (XentPartial)

int xent_lanes(int64_t c) {
  int g = 1;
  while (g < kXentMaxLanes && (int64_t)g * kXentLaneElems < c) g <<= 1;
  return g;
}
unsigned xent_blocks(int64_t n, int g) {
  const int64_t b = ceil_div64(n, kBlock / g);
  return (unsigned)(b < 1 ? 1 : (b > kXentMaxBlocks ? kXentMaxBlocks : b));
}

// exp for the streaming passes: the hardware's exp2 of x * log2(e) (two instructions; relative error about (|x| + 1) * 2^-23, so
// 1e-6 at |x| = 8, where a term still weighs 3e-4 of its sum; exact at 0; 0 below -88).  The ordinary expf costs six times as many,
// and at 349 classes the forward is bound by its instruction stream, not by memory.
__device__ __forceinline__ float xent_exp(float x) { return __expf(x); }

// the single elements before the first aligned piece of row `row`, the pieces, and where the single elements of its end begin
__device__ __forceinline__ void xent_split(idx_t row, idx_t c, idx_t& head, idx_t& nvec, idx_t& tail0) {
  head = (4 - ((row * c) & 3)) & 3;
  if (head > c) head = c;
  nvec = (c - head) >> 2;
  tail0 = head + (nvec << 2);
}

// take(v, j) for the columns j = l, l + G, ... (in pieces of 4) of the row at zr, each column once, in increasing j per lane
template <int G, typename T, typename F>
__device__ __forceinline__ void xent_scan(const T* __restrict__ zr, idx_t row, idx_t c, int l, F&& take) {
  idx_t head, nvec, tail0;
  xent_split(row, c, head, nvec, tail0);
  for (idx_t j = l; j < head; j += G) take(to_f32(zr[j]), j);
  for (idx_t k = l; k < nvec; k += G) {
    const idx_t j = head + (k << 2);
    const float4 v = ldrow4(zr + j);
    take(v.x, j);
    take(v.y, j + 1);
    take(v.z, j + 2);
    take(v.w, j + 3);
  }
  for (idx_t j = tail0 + l; j < c; j += G) take(to_f32(zr[j]), j);
}

// ---- the ordinary row: finite logits and -inf, at least one above -FLT_MAX.  A lane keeps its running maximum m (from -FLT_MAX, so
// that -inf - m is -inf and adds 0 without a test), the sum s of exp relative to it and the first column mi of that maximum; a NaN
// makes s a NaN, +inf makes m +inf, a row of -inf leaves s 0 and mi unset: such a row is done again by the careful scan below.
__device__ __forceinline__ void xent_take(float v, idx_t j, float& m, float& s, idx_t& mi) {
  const float e = xent_exp(-fabsf(v - m));
  const bool gt = v > m;
  s = gt ? s * e + 1.f : s + e;
  m = fmaxf(m, v);
  mi = gt ? j : mi;
}

constexpr int kXentBeaten = 1, kXentNoLse = 2;

// ---- the careful scan (rows holding a NaN or +inf, rows of -inf): one logit into (max, sum); -inf adds nothing; a NaN or +inf is
// flagged (the row's lse is NaN, as max + log(sum(exp(z - max))) gives); `beaten`: the label's logit is not the row's first maximum,
// a NaN ordered above everything
__device__ __forceinline__ void xent_take_careful(float v, idx_t j, float zl, bool zl_nan, idx_t lab, float& m, float& s, int& flags) {
  const bool lower = j < lab;
  const bool beats = zl_nan ? (v != v && lower) : (!(v <= zl) || (v == zl && lower));
  flags |= (beats ? kXentBeaten : 0) | (!(v < INFINITY) ? kXentNoLse : 0);
  if (v != -INFINITY) {
    const float e = expf(-fabsf(v - m));
    if (v > m) {
      s = s * e + 1.f;
      m = v;
    } else {
      s += e;
    }
  }
}

struct XentPartial {  // what a wave leaves for the finish (kXentPartialBytes)
  double loss;
  idx_t valid, correct, bad;
};

template <typename T, int G>
__global__ __launch_bounds__(kBlock) void HET_softmax_xent(const T* __restrict__ z, const idx_t* __restrict__ labels, idx_t n, idx_t c,
                                                           idx_t ignore, float* __restrict__ lse, XentPartial* __restrict__ partials) {
  constexpr int RPW = HET_WAVE / G, RPB = kBlock / G;
  const int lane = threadIdx.x & (HET_WAVE - 1), wave = threadIdx.x / HET_WAVE;
  const int gi = lane / G, l = lane % G;
  const idx_t step = (idx_t)gridDim.x * RPB;
  double acc = 0.0;
  idx_t n_valid = 0, n_correct = 0, n_bad = 0;
  idx_t r0 = (idx_t)blockIdx.x * RPB + wave * RPW;  // (the same in every lane of the wave)
  idx_t lab_next = r0 + gi < n ? labels[r0 + gi] : ignore;
  for (; r0 < n; r0 += step) {
    const idx_t row = r0 + gi;
    const bool in = row < n;
    const idx_t lab = lab_next;
    lab_next = row + step < n ? labels[row + step] : ignore;  // (asked for before this row's logits: one wait less per row)
    const bool ok = in && lab != ignore && lab >= 0 && lab < c;
    const T* zr = z + row * c;
    float m = -FLT_MAX, s = 0.f, zl = 0.f;
    idx_t mi = -1;
    if (ok) {
      zl = to_f32(zr[lab]);
      xent_scan<G>(zr, row, c, l, [&](float v, idx_t j) { xent_take(v, j, m, s, mi); });
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {  // the G lanes of a row (every lane of the wave takes part; skipped rows carry nothing)
      const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
      const idx_t mi2 = __shfl_xor(mi, o);
      const float nm = fmaxf(m, m2);
      s = s * xent_exp(m - nm) + s2 * xent_exp(m2 - nm);
      mi = (m2 > m || (m2 == m && (uint64_t)mi2 < (uint64_t)mi)) ? mi2 : mi;  // (unset = -1 loses to every column)
      m = nm;
    }
    float ls = logf(s);
    bool correct = mi == lab;
    const bool again = ok && (!(s > 0.f) || m == INFINITY || mi < 0);  // (the same in the G lanes of a row up to the order of a sum: see below)
    if (__any(again)) {
      // `again` is taken from lane 0 of the row: the butterfly adds in another order in every lane, so s may differ in its last bit
      const bool redo = __shfl(again ? 1 : 0, gi * G) != 0;
      float cm = -INFINITY, cs = 0.f;
      int flags = 0;
      if (redo) {
        const bool zl_nan = zl != zl;
        xent_scan<G>(zr, row, c, l, [&](float v, idx_t j) { xent_take_careful(v, j, zl, zl_nan, lab, cm, cs, flags); });
      }
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(cm, o), s2 = __shfl_xor(cs, o);
        flags |= __shfl_xor(flags, o);
        const float nm = fmaxf(cm, m2);
        cs = nm == -INFINITY ? 0.f : cs * expf(cm - nm) + s2 * expf(m2 - nm);
        cm = nm;
      }
      if (redo) {
        if ((flags & kXentNoLse) || cm == -INFINITY) cs = NAN;
        m = cm;
        ls = logf(cs);
        correct = !(flags & kXentBeaten);
      }
    }
    if (l == 0 && in) {
      float row_lse = 0.f;
      if (ok) {
        row_lse = m + ls;
        acc += (double)(ls + (m - zl));
        n_valid += 1;
        n_correct += correct ? 1 : 0;
      } else if (lab != ignore) {
        n_bad += 1;
      }
      if (lse) lse[row] = row_lse;
    }
  }
#pragma unroll
  for (int o = HET_WAVE / 2; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o);
    n_valid += __shfl_xor(n_valid, o);
    n_correct += __shfl_xor(n_correct, o);
    n_bad += __shfl_xor(n_bad, o);
  }
  if (lane == 0)  // every wave of the grid stores its partial, rows or not: the finish reads all of them
    partials[(idx_t)blockIdx.x * kXentWavesPerBlock + wave] = XentPartial{acc, n_valid, n_correct, n_bad};
}

// one wave: lane i adds the partials i, i + 64, ... in that order (kXentFinishBatch loads in flight at a time), a butterfly adds the lanes
constexpr int kXentFinishBatch = 16;
__global__ __launch_bounds__(HET_WAVE) void HET_softmax_xent_finish(const XentPartial* __restrict__ partials, idx_t waves, int mean,
                                                                   float* __restrict__ loss, idx_t* __restrict__ stats) {
  double acc = 0.0;
  idx_t n_valid = 0, n_correct = 0, n_bad = 0;
  for (idx_t w0 = threadIdx.x; w0 < waves; w0 += (idx_t)HET_WAVE * kXentFinishBatch) {
    XentPartial p[kXentFinishBatch];
#pragma unroll
    for (int u = 0; u < kXentFinishBatch; ++u) {
      const idx_t w = w0 + (idx_t)u * HET_WAVE;
      p[u] = w < waves ? partials[w] : XentPartial{0.0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < kXentFinishBatch; ++u) {
      acc += p[u].loss;
      n_valid += p[u].valid;
      n_correct += p[u].correct;
      n_bad += p[u].bad;
    }
  }
#pragma unroll
  for (int o = HET_WAVE / 2; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o);
    n_valid += __shfl_xor(n_valid, o);
    n_correct += __shfl_xor(n_correct, o);
    n_bad += __shfl_xor(n_bad, o);
  }
  if (threadIdx.x == 0) {
    *loss = (float)(mean ? acc / (double)n_valid : acc);  // (no valid row: 0 / 0, a NaN, as torch's mean gives)
    stats[0] = n_valid;
    stats[1] = n_correct;
    stats[2] = n_bad;
  }
}

__device__ __forceinline__ float xent_grad1(float v, float row_lse, bool at_label, float gs) {
  return (xent_exp(v - row_lse) - (at_label ? 1.f : 0.f)) * gs;
}

template <typename T, int G>
__global__ __launch_bounds__(kBlock) void HET_softmax_xent_backward(const T* __restrict__ z, const idx_t* __restrict__ labels,
                                                                    const float* __restrict__ lse, const idx_t* __restrict__ stats,
                                                                    const float* __restrict__ grad_loss, idx_t n, idx_t c, idx_t ignore,
                                                                    int mean, T* __restrict__ gz) {
  constexpr int RPB = kBlock / G;
  const int gi = threadIdx.x / G, l = threadIdx.x % G;
  const idx_t step = (idx_t)gridDim.x * RPB;
  const float gs = mean ? *grad_loss / (float)stats[0] : *grad_loss;  // (no valid row: never used)
  idx_t row = (idx_t)blockIdx.x * RPB + gi;
  idx_t lab_next = row < n ? labels[row] : ignore;
  for (; row < n; row += step) {
    const idx_t lab = lab_next;
    lab_next = row + step < n ? labels[row + step] : ignore;  // (asked for before this row's logits)
    const bool ok = lab != ignore && lab >= 0 && lab < c;
    const T* zr = z + row * c;
    T* gr = gz + row * c;
    idx_t head, nvec, tail0;
    xent_split(row, c, head, nvec, tail0);
    if (ok) {
      const float row_lse = lse[row];
      for (idx_t j = l; j < head; j += G) strow1(gr + j, xent_grad1(to_f32(zr[j]), row_lse, j == lab, gs));
      for (idx_t k = l; k < nvec; k += G) {
        const idx_t j = head + (k << 2);
        const float4 v = ldrow4(zr + j);
        strow4(gr + j, make_float4(xent_grad1(v.x, row_lse, j == lab, gs), xent_grad1(v.y, row_lse, j + 1 == lab, gs),
                                   xent_grad1(v.z, row_lse, j + 2 == lab, gs), xent_grad1(v.w, row_lse, j + 3 == lab, gs)));
      }
      for (idx_t j = tail0 + l; j < c; j += G) strow1(gr + j, xent_grad1(to_f32(zr[j]), row_lse, j == lab, gs));
    } else {  // a skipped row: +0 everywhere, its logits are not read
      for (idx_t j = l; j < head; j += G) strow1(gr + j, 0.f);
      for (idx_t k = l; k < nvec; k += G) strow4(gr + head + (k << 2), make_float4(0.f, 0.f, 0.f, 0.f));
      for (idx_t j = tail0 + l; j < c; j += G) strow1(gr + j, 0.f);
    }
  }
}

// the checks the entries share; -1 = nothing to do (n == 0)
template <typename T>
int xent_check(const char* op, const T* logits, const int64_t* labels, int64_t n, int64_t c, int reduction) {
  HET_REQUIRE(n >= 0, "%s: n=%lld", op, (long long)n);
  HET_REQUIRE(c >= 1, "%s: c=%lld (at least one class)", op, (long long)c);
  if (reduction != HET_XENT_MEAN && reduction != HET_XENT_SUM) {
    het_set_error("%s: reduction %d (0 = mean, 1 = sum)", op, reduction);
    return HET_ERR_UNSUPPORTED;
  }
  if (n == 0) return -1;
  HET_REQUIRE(n <= (INT64_MAX / 8) / c, "%s: n=%lld rows of c=%lld logits are beyond a 64-bit byte offset", op, (long long)n, (long long)c);
  HET_REQUIRE(logits && labels, "%s: null pointer", op);
  HET_REQUIRE((sizeof(T) == 4 ? aligned16(logits) : aligned8(logits)) && aligned8(labels),
              "%s: misaligned pointer (logits on %d-byte, labels on 8-byte boundaries)", op, (int)(4 * sizeof(T)));
  return HET_OK;
}

template <typename T>
int softmax_xent(const char* op, const T* logits, const int64_t* labels, int64_t n, int64_t c, int64_t ignore_index, int reduction, float* loss,
                 float* lse, int64_t* stats, void* workspace, int64_t workspace_bytes, het_stream stream) {
  const int rc = xent_check(op, logits, labels, n, c, reduction);
  if (rc != HET_OK) return rc < 0 ? HET_OK : rc;
  HET_REQUIRE(loss && stats, "%s: null pointer", op);
  HET_REQUIRE(((uintptr_t)loss & 3) == 0 && ((uintptr_t)lse & 3) == 0 && aligned8(stats, workspace),
              "%s: misaligned pointer (loss and lse on 4-byte, stats and workspace on 8-byte boundaries)", op);
  const int g = xent_lanes(c);
  const unsigned blocks = xent_blocks(n, g);
  const int64_t waves = (int64_t)blocks * kXentWavesPerBlock;
  HET_REQUIRE(workspace && workspace_bytes >= waves * kXentPartialBytes, "%s: workspace of %lld bytes, %lld needed (het_softmax_xent_workspace)",
              op, (long long)(workspace ? workspace_bytes : 0), (long long)(waves * kXentPartialBytes));
  hipStream_t s = (hipStream_t)stream;
  XentPartial* partials = (XentPartial*)workspace;
  {
    HET_KTIME("HET_softmax_xent", s);
    HET_DISPATCH_LPR(g, hipLaunchKernelGGL((HET_softmax_xent<T, LPR>), dim3(blocks), dim3(kBlock), 0, s, logits, (const idx_t*)labels, (idx_t)n,
                                           (idx_t)c, (idx_t)ignore_index, lse, partials));
    HET_LAUNCH_CHECK("HET_softmax_xent");
  }
  HET_KTIME("HET_softmax_xent_finish", s);
  hipLaunchKernelGGL(HET_softmax_xent_finish, dim3(1), dim3(HET_WAVE), 0, s, (const XentPartial*)partials, (idx_t)waves,
                     (int)(reduction == HET_XENT_MEAN), loss, (idx_t*)stats);
  HET_LAUNCH_CHECK("HET_softmax_xent_finish");
  return HET_OK;
}

template <typename T>
int softmax_xent_backward(const char* op, const T* logits, const int64_t* labels, const float* lse, const int64_t* stats, const float* grad_loss,
                          int64_t n, int64_t c, int64_t ignore_index, int reduction, T* grad_logits, het_stream stream) {
  const int rc = xent_check(op, logits, labels, n, c, reduction);
  if (rc != HET_OK) return rc < 0 ? HET_OK : rc;
  HET_REQUIRE(lse && stats && grad_loss && grad_logits, "%s: null pointer", op);
  HET_REQUIRE((sizeof(T) == 4 ? aligned16(grad_logits) : aligned8(grad_logits)) && (((uintptr_t)lse | (uintptr_t)grad_loss) & 3) == 0 && aligned8(stats),
              "%s: misaligned pointer (grad_logits on %d-byte, lse and grad_loss on 4-byte, stats on 8-byte boundaries)", op, (int)(4 * sizeof(T)));
  const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)grad_logits, bytes = (uintptr_t)n * (uintptr_t)c * sizeof(T);
  HET_REQUIRE(!(a < b + bytes && b < a + bytes), "%s: grad_logits overlaps logits (not an in-place operation)", op);
  hipStream_t s = (hipStream_t)stream;
  const int g = xent_lanes(c);
  const unsigned blocks = xent_blocks(n, g);
  HET_KTIME("HET_softmax_xent_backward", s);
  HET_DISPATCH_LPR(g, hipLaunchKernelGGL((HET_softmax_xent_backward<T, LPR>), dim3(blocks), dim3(kBlock), 0, s, logits, (const idx_t*)labels, lse,
                                         (const idx_t*)stats, grad_loss, (idx_t)n, (idx_t)c, (idx_t)ignore_index,
                                         (int)(reduction == HET_XENT_MEAN), grad_logits));
  HET_LAUNCH_CHECK("HET_softmax_xent_backward");
  return HET_OK;
}

}  // namespace

extern "C" int het_softmax_xent_params(int64_t* out) {
  HET_REQUIRE(out, "het_softmax_xent_params: null pointer");
  out[0] = kXentLaneElems;
  out[1] = kXentMaxLanes;
  out[2] = kXentMaxBlocks;
  out[3] = kBlock;
  return HET_OK;
}

extern "C" int64_t het_softmax_xent_workspace(int64_t n, int64_t c) {
  if (n < 0 || c < 1) {
    het_set_error("het_softmax_xent_workspace: n=%lld, c=%lld", (long long)n, (long long)c);
    return -1;
  }
  return n == 0 ? 0 : (int64_t)xent_blocks(n, xent_lanes(c)) * kXentWavesPerBlock * kXentPartialBytes;
}

extern "C" int het_softmax_xent(const float* logits, const int64_t* labels, int64_t n, int64_t c, int64_t ignore_index, int reduction,
                                float* loss, float* lse, int64_t* stats, void* workspace, int64_t workspace_bytes, het_stream stream) {
  return softmax_xent("het_softmax_xent", logits, labels, n, c, ignore_index, reduction, loss, lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int het_softmax_xent_bf16(const het_bf16* logits, const int64_t* labels, int64_t n, int64_t c, int64_t ignore_index, int reduction,
                                     float* loss, float* lse, int64_t* stats, void* workspace, int64_t workspace_bytes, het_stream stream) {
  return softmax_xent("het_softmax_xent_bf16", logits, labels, n, c, ignore_index, reduction, loss, lse, stats, workspace, workspace_bytes, stream);
}

extern "C" int het_softmax_xent_backward(const float* logits, const int64_t* labels, const float* lse, const int64_t* stats,
                                         const float* grad_loss, int64_t n, int64_t c, int64_t ignore_index, int reduction,
                                         float* grad_logits, het_stream stream) {
  return softmax_xent_backward("het_softmax_xent_backward", logits, labels, lse, stats, grad_loss, n, c, ignore_index, reduction, grad_logits,
                               stream);
}

extern "C" int het_softmax_xent_backward_bf16(const het_bf16* logits, const int64_t* labels, const float* lse, const int64_t* stats,
                                              const float* grad_loss, int64_t n, int64_t c, int64_t ignore_index, int reduction,
                                              het_bf16* grad_logits, het_stream stream) {
  return softmax_xent_backward("het_softmax_xent_backward_bf16", logits, labels, lse, stats, grad_loss, n, c, ignore_index, reduction,
                               grad_logits, stream);
}
