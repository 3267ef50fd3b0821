// Row-sparse access to a learnable [N, K] fp32 table (HET_RelGraphEmbed.embeds) for sampled mini-batches: the rows a block names are
// gathered (optionally rounded to bf16 at the store), and a lazy Adam step updates only the rows a sparse gradient names.
//
//   HET_rows_embed_gather   out[i, :] = table[rows[i], :]                                      i in [0, B)
//   HET_rows_adam           for every run of equal ids in rows_sorted (ascending, repeats allowed):
//                             g = SUM over the run's positions j, in position order, of grad[perm[j], :]
//                             m = b1 m + (1 - b1) g    v = b2 v + (1 - b2) g g    p -= step_size m / (sqrt(v) + eps)
//                           step_size = lr sqrt(bias_correction2) / bias_correction1 -- torch.optim.SparseAdam's rule: eps is added to
//                           sqrt(v), not to sqrt(v / bias_correction2) as dense Adam does, and rows outside the gradient keep p, m, v.
//
// Both are bound by the rate of scattered 4K-byte rows: a row is covered by a lane group of L lanes, the smallest
// power of two >= K/4 (64 at most), every lane moving 16 bytes per access; lane l holds the float4s l, l + L, ... (more than one only
// above K = 256).  Row offsets are 64-bit: N * K passes 2^31 on tables of a few GB.
//
// The Adam pass uses no atomics and no scratch: the lane group at sorted position j works only when j is the head of its run
// (j == 0 or rows_sorted[j] != rows_sorted[j-1]); it walks the run to its end -- past the positions of its own workgroup if the run
// is that long -- and adds the gradient rows in position order in registers, so a run is summed by one lane group in one fixed order
// and the result is the same bits every launch.  Every row of p, m, v is read and written by exactly one lane group.
// Square root and division are the correctly rounded ones (no fast-math flag in this build, no rsqrt / rcp builtins): the state
// compounds over thousands of steps.
#include "common.hip.h"

namespace {

constexpr int kEmbedMaxK = 1024;

inline bool embed_shape_ok(int64_t K) { return K >= 4 && K <= kEmbedMaxK && K % 4 == 0; }

// lanes per row: the smallest power of two that covers the row's float4s, 64 at most
inline int embed_lanes(int64_t K) {
  int l = 1;
  while (l < 64 && l < K / 4) l *= 2;
  return l;
}

// An id outside [0, N) is never turned into an address: the gather writes a row of zeros for it, the Adam pass skips its run.
template <typename T, int L>
__global__ __launch_bounds__(256) void HET_rows_embed_gather(const float* __restrict__ table, const idx_t* __restrict__ rows, idx_t B,
                                                             idx_t N, int K4, T* __restrict__ out) {
  constexpr int G = 256 / L;  // lane groups (rows in flight) per workgroup
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const idx_t K = (idx_t)K4 * 4;
  for (idx_t i = (idx_t)blockIdx.x * G + g; i < B; i += (idx_t)gridDim.x * G) {
    const idx_t r = rows[i];
    const bool ok = (uint64_t)r < (uint64_t)N;
    const float* src = table + (ok ? r : 0) * K;
    T* dst = out + i * K;
    for (int c = l; c < K4; c += L) strow4(dst + 4 * c, ok ? ld4(src + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

template <int L>
__global__ __launch_bounds__(256) void HET_rows_adam(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                     const idx_t* __restrict__ rows_sorted, const idx_t* __restrict__ perm,
                                                     const float* __restrict__ grad, idx_t B, idx_t N, int K4, float b1, float b2,
                                                     float omb1, float omb2, float step_size, float eps) {
  constexpr int G = 256 / L;
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const idx_t K = (idx_t)K4 * 4;
  for (idx_t j = (idx_t)blockIdx.x * G + g; j < B; j += (idx_t)gridDim.x * G) {
    const idx_t r = rows_sorted[j];
    if (j > 0 && rows_sorted[j - 1] == r) continue;  // (not the head of its run: the head does this position's work)
    if ((uint64_t)r >= (uint64_t)N) continue;
    for (int c = l; c < K4; c += L) {
      float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
      for (idx_t q = j; q < B && rows_sorted[q] == r; ++q) {
        const idx_t gi = perm ? perm[q] : q;
        if ((uint64_t)gi >= (uint64_t)B) continue;  // (a perm that is no permutation of 0 .. B-1: nothing outside grad is read)
        const float4 t = ld4(grad + gi * K + 4 * c);
        gs.x += t.x; gs.y += t.y; gs.z += t.z; gs.w += t.w;
      }
      const idx_t off = r * K + 4 * c;
      float4 mm = ld4(m + off), vv = ld4(v + off), pp = ld4(p + off);
      mm = make_float4(b1 * mm.x + omb1 * gs.x, b1 * mm.y + omb1 * gs.y, b1 * mm.z + omb1 * gs.z, b1 * mm.w + omb1 * gs.w);
      vv = make_float4(b2 * vv.x + omb2 * gs.x * gs.x, b2 * vv.y + omb2 * gs.y * gs.y, b2 * vv.z + omb2 * gs.z * gs.z,
                       b2 * vv.w + omb2 * gs.w * gs.w);
      pp = make_float4(pp.x - step_size * (mm.x / (sqrtf(vv.x) + eps)), pp.y - step_size * (mm.y / (sqrtf(vv.y) + eps)),
                       pp.z - step_size * (mm.z / (sqrtf(vv.z) + eps)), pp.w - step_size * (mm.w / (sqrtf(vv.w) + eps)));
      st4(m + off, mm);
      st4(v + off, vv);
      st4(p + off, pp);
    }
  }
}

// workgroups of a launch with one lane group of L lanes per position: every position gets a lane group up to 16 K workgroups,
// grid-stride above
inline unsigned embed_grid(int64_t B, int L) { return grid_for(B * L); }

template <typename T, int L, typename... A>
void embed_launch_gather(unsigned blocks, hipStream_t s, A... args) {
  hipLaunchKernelGGL((HET_rows_embed_gather<T, L>), dim3(blocks), dim3(256), 0, s, args...);
}
template <int L, typename... A>
void embed_launch_adam(unsigned blocks, hipStream_t s, A... args) {
  hipLaunchKernelGGL((HET_rows_adam<L>), dim3(blocks), dim3(256), 0, s, args...);
}

template <typename T>
int rows_embed_gather(const char* op, const float* table, const int64_t* rows, int64_t B, int64_t N, int64_t K, T* out,
                      het_stream stream) {
  HET_REQUIRE(B >= 0 && N >= 0 && K > 0, "%s: bad arguments", op);
  if (!embed_shape_ok(K)) {
    het_set_error("%s: rows of 4 .. %d floats, a multiple of 4 (K=%lld)", op, kEmbedMaxK, (long long)K);
    return HET_ERR_UNSUPPORTED;
  }
  if (B == 0) return HET_OK;
  HET_REQUIRE(table && rows && out, "%s: null pointer", op);
  HET_REQUIRE(aligned16(table) && (sizeof(T) == 4 ? aligned16(out) : aligned8(out)) && aligned8(rows),
              "%s: misaligned pointer (table 16 bytes, out %d bytes, rows 8 bytes)", op, (int)(4 * sizeof(T)));
  const int lanes = embed_lanes(K);
  HET_KTIME("HET_rows_embed_gather", (hipStream_t)stream);
  HET_DISPATCH_LPR(lanes, (embed_launch_gather<T, LPR>(embed_grid(B, lanes), (hipStream_t)stream, table, rows, (idx_t)B, (idx_t)N,
                                                       (int)(K / 4), out)));
  HET_LAUNCH_CHECK("HET_rows_embed_gather");
  return HET_OK;
}
}  // namespace

extern "C" int het_rows_embed_ok(int64_t K) { return embed_shape_ok(K) ? 1 : 0; }

extern "C" int het_rows_embed_gather(const float* table, const int64_t* rows, int64_t num_rows, int64_t num_table_rows, int64_t K,
                                     float* out, het_stream stream) {
  return rows_embed_gather("het_rows_embed_gather", table, rows, num_rows, num_table_rows, K, out, stream);
}

extern "C" int het_rows_embed_gather_bf16(const float* table, const int64_t* rows, int64_t num_rows, int64_t num_table_rows, int64_t K,
                                          het_bf16* out, het_stream stream) {
  return rows_embed_gather("het_rows_embed_gather_bf16", table, rows, num_rows, num_table_rows, K, out, stream);
}

extern "C" int het_rows_adam(float* p, float* m, float* v, const int64_t* rows_sorted, const int64_t* perm, const float* grad,
                             int64_t num_rows, int64_t num_table_rows, int64_t K, double lr, double beta1, double beta2, double eps,
                             double bias_correction1, double bias_correction2, het_stream stream) {
  const char* op = "het_rows_adam";
  HET_REQUIRE(num_rows >= 0 && num_table_rows >= 0 && K > 0, "%s: bad arguments", op);
  HET_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && bias_correction1 > 0.0 &&
                  bias_correction2 > 0.0,
              "%s: lr >= 0, betas in [0, 1), eps >= 0 and positive bias corrections expected", op);
  if (!embed_shape_ok(K)) {
    het_set_error("%s: rows of 4 .. %d floats, a multiple of 4 (K=%lld)", op, kEmbedMaxK, (long long)K);
    return HET_ERR_UNSUPPORTED;
  }
  if (num_rows == 0) return HET_OK;
  HET_REQUIRE(p && m && v && rows_sorted && grad, "%s: null pointer", op);
  HET_REQUIRE(aligned16(p, m, v, grad) && aligned8(rows_sorted, perm), "%s: misaligned pointer (fp32 tensors 16 bytes, id lists 8 bytes)", op);
  const double step_size = lr * sqrt(bias_correction2) / bias_correction1;
  const int lanes = embed_lanes(K);
  HET_KTIME("HET_rows_adam", (hipStream_t)stream);
  HET_DISPATCH_LPR(lanes, (embed_launch_adam<LPR>(embed_grid(num_rows, lanes), (hipStream_t)stream, p, m, v, rows_sorted, perm, grad,
                                                  (idx_t)num_rows, (idx_t)num_table_rows, (int)(K / 4), (float)beta1, (float)beta2,
                                                  (float)(1.0 - beta1), (float)(1.0 - beta2), (float)step_size, (float)eps)));
  HET_LAUNCH_CHECK("HET_rows_adam");
  return HET_OK;
}
