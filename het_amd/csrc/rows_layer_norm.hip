// Typed LayerNorm over the rows of a [N, X] tensor (HGT's use_norm: x = norm_t(W[t] . Agg(x)), one affine pair per node type).
//
//   mean_v = SUM_j y[v,j] / X      var_v = SUM_j (y[v,j] - mean_v)^2 / X      rstd_v = 1 / sqrt(var_v + eps)
//   out[v,:] = (y[v,:] - mean_v) * rstd_v * gamma[t(v),:] + beta[t(v),:]       t(v): the run of offsets [T+1] that holds row v
//
// A memory-bound sweep: every row is read once and held in registers between the mean, the variance (the mean of the squared
// deviations from the mean -- not E[y^2] - mean^2, which cancels where |mean| >> std) and the store.  A row of X floats is covered
// by L lanes, a power of two <= 64, lane l holding the float4s l, l + L, ... (V of them; V > 1 only at L = 64): X = 64 is 16 lanes
// and 4 rows per wave, X = 8 is 2 lanes and 32 rows per wave, X = 1024 is 64 lanes of 4 float4s.  Widths that are no power of two
// take the next L up with the lanes past the row's end switched off (X = 100: 25 of 32 lanes).  The sums are butterflies inside
// the lane group (every lane of the group ends with the same bits), no LDS.
//
// A workgroup works on a tile of rows of ONE type (tile_to_relation), so gamma / beta stay in registers for the tile, and in the
// backward the column sums of the parameter gradients stay in registers across the tile's rows: they meet the other lane groups
// of the wave by butterfly, the other waves in LDS, and leave as one partial row pair [2, X] per tile.  HET_rows_layer_norm_colsum
// adds the partials of a type in a fixed order: no float atomics, the parameter gradients are the same bits every run.
#include "common.hip.h"

namespace {

constexpr int kLnMaxX = 1024;

inline bool ln_shape_ok(int64_t X) { return X >= 4 && X <= kLnMaxX && X % 4 == 0; }

// lanes per row: the smallest power of two that covers the row's float4s, 64 at most
inline int ln_lanes(int64_t X) {
  int l = 1;
  while (l < 64 && l < X / 4) l *= 2;
  return l;
}

// rows per tile: 256 (a workgroup's lane groups at X = 4) doubled until a launch has no more than ~2048 tiles
inline int64_t ln_tile_rows(int64_t num_rows) {
  int64_t t = 256;
  while (t * 2048 < num_rows && t < (1ll << 30)) t *= 2;
  return t;
}
// an upper bound of the tiles of any offsets [T+1] over num_rows rows (every run may end with a partial tile)
inline int64_t ln_max_tiles(int64_t num_rows, int64_t num_types) { return ceil_div64(num_rows, ln_tile_rows(num_rows)) + num_types; }

template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = L / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// ... of the same lane of every lane group of the wave
template <int L>
__device__ __forceinline__ float across_groups_sum(float v) {
#pragma unroll
  for (int o = L; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float hsum(float4 v) { return (v.x + v.y) + (v.z + v.w); }
// pairwise over the lane's float4s (a constant row of a power-of-two width sums exactly)
template <int V>
__device__ __forceinline__ float tree_sum(const float (&s)[V]) {
  if constexpr (V == 1) return s[0];
  else if constexpr (V == 2) return s[0] + s[1];
  else if constexpr (V == 3) return (s[0] + s[1]) + s[2];
  else return (s[0] + s[1]) + (s[2] + s[3]);
}

// the tile of this workgroup clipped to [0, num_rows): false when the launch has more workgroups than the offsets have tiles
__device__ __forceinline__ bool ln_tile(const idx_t* __restrict__ offsets, int T, int tile_rows, idx_t num_rows, int& t,
                                        idx_t& row_begin, idx_t& row_end) {
  if (!tile_to_relation(offsets, T, tile_rows, (long)blockIdx.x, t, row_begin, row_end)) return false;
  if (row_begin < 0) row_begin = 0;
  if (row_end > num_rows) row_end = num_rows;
  return true;
}

template <typename T, int L, int V>
__global__ __launch_bounds__(256) void HET_rows_layer_norm(const idx_t* __restrict__ offsets, int num_types, int tile_rows,
                                                           const T* __restrict__ y, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, T* __restrict__ out,
                                                           float* __restrict__ mean, float* __restrict__ rstd, idx_t num_rows,
                                                           int X) {
  constexpr int G = 256 / L;  // lane groups (rows in flight) per workgroup
  int t;
  idx_t row_begin, row_end;
  if (!ln_tile(offsets, num_types, tile_rows, num_rows, t, row_begin, row_end)) return;
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const int X4 = X >> 2;
  const float inv_x = 1.f / (float)X;
  bool on[V];
  float4 gm[V], bt[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = l + j * L;
    on[j] = c < X4;
    gm[j] = on[j] ? ld4(gamma + (idx_t)t * X + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    bt[j] = on[j] ? ld4(beta + (idx_t)t * X + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (idx_t base = row_begin; base < row_end; base += G) {  // (the same trip count in every lane: the butterflies are whole)
    const idx_t row = base + g;
    const bool valid = row < row_end;
    float4 v[V];
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      v[j] = valid && on[j] ? ldrow4(y + row * X + 4 * (l + j * L)) : make_float4(0.f, 0.f, 0.f, 0.f);
      s[j] = hsum(v[j]);
    }
    const float mu = group_sum<L>(tree_sum<V>(s)) * inv_x;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      v[j] = on[j] ? make_float4(v[j].x - mu, v[j].y - mu, v[j].z - mu, v[j].w - mu) : v[j];
      s[j] = hsum(make_float4(v[j].x * v[j].x, v[j].y * v[j].y, v[j].z * v[j].z, v[j].w * v[j].w));
    }
    const float rs = rsqrtf(group_sum<L>(tree_sum<V>(s)) * inv_x + eps);
    if (!valid) continue;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (!on[j]) continue;
      const float4 o = make_float4(v[j].x * rs * gm[j].x + bt[j].x, v[j].y * rs * gm[j].y + bt[j].y,
                                   v[j].z * rs * gm[j].z + bt[j].z, v[j].w * rs * gm[j].w + bt[j].w);
      strow4(out + row * X + 4 * (l + j * L), o);
    }
    if (l == 0 && mean) {  // (mean and rstd come and go together: the host checks)
      mean[row] = mu;
      rstd[row] = rs;
    }
  }
}

// grad_y = rstd * (a - mean_j(a) - xhat * mean_j(a * xhat)),  a = grad_out * gamma[t],  xhat = (y - mean) * rstd -- from y, never
// from out (which would divide by gamma).  partial[tile] = [SUM_v grad_out * xhat | SUM_v grad_out] over the tile's rows.
template <typename T, int L, int V>
__global__ __launch_bounds__(256) void HET_rows_layer_norm_backward(const idx_t* __restrict__ offsets, int num_types, int tile_rows,
                                                                    const T* __restrict__ y, const float* __restrict__ gamma,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const T* __restrict__ grad_out, T* __restrict__ grad_y,
                                                                    float* __restrict__ partial, idx_t num_rows, int X) {
  constexpr int G = 256 / L;
  __shared__ float4 sh[4][2][V][L];  // per wave: the two column sums of its lane groups
  int t;
  idx_t row_begin, row_end;
  if (!ln_tile(offsets, num_types, tile_rows, num_rows, t, row_begin, row_end)) return;
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const int X4 = X >> 2;
  const float inv_x = 1.f / (float)X;
  bool on[V];
  float4 gm[V], dg[V], db[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = l + j * L;
    on[j] = c < X4;
    gm[j] = on[j] ? ld4(gamma + (idx_t)t * X + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    dg[j] = db[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (idx_t base = row_begin; base < row_end; base += G) {
    const idx_t row = base + g;
    const bool valid = row < row_end;
    const float mu = valid ? mean[row] : 0.f, rs = valid ? rstd[row] : 0.f;
    float4 xh[V], a[V];
    float s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool ld = valid && on[j];
      const float4 v = ld ? ldrow4(y + row * X + 4 * (l + j * L)) : make_float4(mu, mu, mu, mu);
      const float4 go = ld ? ldrow4(grad_out + row * X + 4 * (l + j * L)) : make_float4(0.f, 0.f, 0.f, 0.f);
      xh[j] = make_float4((v.x - mu) * rs, (v.y - mu) * rs, (v.z - mu) * rs, (v.w - mu) * rs);
      a[j] = make_float4(go.x * gm[j].x, go.y * gm[j].y, go.z * gm[j].z, go.w * gm[j].w);
      s1[j] = hsum(a[j]);
      s2[j] = hsum(make_float4(a[j].x * xh[j].x, a[j].y * xh[j].y, a[j].z * xh[j].z, a[j].w * xh[j].w));
      dg[j].x += go.x * xh[j].x; dg[j].y += go.y * xh[j].y; dg[j].z += go.z * xh[j].z; dg[j].w += go.w * xh[j].w;
      db[j].x += go.x; db[j].y += go.y; db[j].z += go.z; db[j].w += go.w;
    }
    const float ma = group_sum<L>(tree_sum<V>(s1)) * inv_x;
    const float mb = group_sum<L>(tree_sum<V>(s2)) * inv_x;
    if (!valid || !grad_y) continue;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (!on[j]) continue;
      const float4 o = make_float4(rs * (a[j].x - ma - xh[j].x * mb), rs * (a[j].y - ma - xh[j].y * mb),
                                   rs * (a[j].z - ma - xh[j].z * mb), rs * (a[j].w - ma - xh[j].w * mb));
      strow4(grad_y + row * X + 4 * (l + j * L), o);
    }
  }
  // the tile's column sums: lane groups of a wave by butterfly, the four waves in LDS, both in a fixed order
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    dg[j] = make_float4(across_groups_sum<L>(dg[j].x), across_groups_sum<L>(dg[j].y), across_groups_sum<L>(dg[j].z),
                        across_groups_sum<L>(dg[j].w));
    db[j] = make_float4(across_groups_sum<L>(db[j].x), across_groups_sum<L>(db[j].y), across_groups_sum<L>(db[j].z),
                        across_groups_sum<L>(db[j].w));
    if ((threadIdx.x & 63) < L) {
      sh[wave][0][j][l] = dg[j];
      sh[wave][1][j][l] = db[j];
    }
  }
  __syncthreads();
  float* dst = partial + (idx_t)blockIdx.x * 2 * X;
  for (int i = threadIdx.x; i < 2 * V * L; i += 256) {
    const int which = i / (V * L), j = (i / L) % V, ll = i % L;
    const int c = ll + j * L;
    if (c >= X4) continue;
    float4 acc = sh[0][which][j][ll];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 p = sh[w][which][j][ll];
      acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
    }
    st4(dst + (idx_t)which * X + 4 * c, acc);
  }
}

// grad_gamma[t, :] / grad_beta[t, :] = the partials of type t's tiles added in tile order: 16 columns x 16 slices per workgroup,
// slice s taking the tiles s, s + 16, ..., the slices added in LDS in slice order.  A type without rows gets zeros.
__global__ __launch_bounds__(256) void HET_rows_layer_norm_colsum(const idx_t* __restrict__ offsets, int tile_rows,
                                                                  const float* __restrict__ partial, long max_tiles, int X,
                                                                  float* __restrict__ grad_gamma, float* __restrict__ grad_beta) {
  __shared__ float sh[16][16];
  const int t = blockIdx.x, which = blockIdx.z;
  const int cl = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int c = blockIdx.y * 16 + cl;
  long first = 0;
  for (int i = 0; i < t; ++i) first += (offsets[i + 1] - offsets[i] + tile_rows - 1) / tile_rows;  // (as tile_to_relation counts)
  long nt = (offsets[t + 1] - offsets[t] + tile_rows - 1) / tile_rows;
  if (first < 0) first = 0;
  if (first + nt > max_tiles) nt = max_tiles - first;  // (offsets the launch was not sized for: stay inside the workspace)
  float acc = 0.f;
  if (c < X)
    for (long i = s; i < nt; i += 16) acc += partial[((first + i) * 2 + which) * X + c];
  sh[s][cl] = acc;
  __syncthreads();
  if (s == 0 && c < X) {
    float v = sh[0][cl];
#pragma unroll
    for (int k = 1; k < 16; ++k) v += sh[k][cl];
    (which ? grad_beta : grad_gamma)[(idx_t)t * X + c] = v;
  }
}

template <typename T, int L, int V, typename... A>
void ln_launch_forward(unsigned tiles, hipStream_t s, A... args) {
  hipLaunchKernelGGL((HET_rows_layer_norm<T, L, V>), dim3(tiles), dim3(256), 0, s, args...);
}
template <typename T, int L, int V, typename... A>
void ln_launch_backward(unsigned tiles, hipStream_t s, A... args) {
  hipLaunchKernelGGL((HET_rows_layer_norm_backward<T, L, V>), dim3(tiles), dim3(256), 0, s, args...);
}

// FN<T, L, V>(...) with the lanes per row L and the float4s per lane V (V > 1 only at 64 lanes) of width X
#define HET_LN_DISPATCH(X, FN, ...)                                           \
  do {                                                                        \
    const int lanes__ = ln_lanes(X);                                          \
    const int v__ = (int)ceil_div64((X) / 4, lanes__);                        \
    if (lanes__ == 64 && v__ == 2) FN<T, 64, 2>(__VA_ARGS__);                 \
    else if (lanes__ == 64 && v__ == 3) FN<T, 64, 3>(__VA_ARGS__);            \
    else if (lanes__ == 64 && v__ == 4) FN<T, 64, 4>(__VA_ARGS__);            \
    else HET_DISPATCH_LPR(lanes__, (FN<T, LPR, 1>(__VA_ARGS__)));             \
  } while (0)

template <typename T>
bool ln_rows_aligned(const T* a, const T* b) { return sizeof(T) == 4 ? aligned16(a, b) : aligned8(a, b); }

template <typename T>
int rows_layer_norm(const char* op, const int64_t* offsets, int64_t num_types, const T* y, const float* gamma, const float* beta,
                    double eps, T* out, float* mean, float* rstd, int64_t num_rows, int64_t X, het_stream stream) {
  HET_REQUIRE(offsets && num_types > 0 && num_types < (1ll << 31) && num_rows >= 0 && X > 0 && eps >= 0.0, "%s: bad arguments", op);
  HET_REQUIRE((mean == nullptr) == (rstd == nullptr), "%s: mean and rstd are both given or both NULL", op);
  if (num_rows == 0) return HET_OK;
  HET_REQUIRE(y && gamma && beta && out, "%s: null data pointer", op);
  if (!(ln_shape_ok(X) && ln_rows_aligned(y, (const T*)out) && aligned16(gamma, beta) && ((uintptr_t)mean & 3) == 0 &&
        ((uintptr_t)rstd & 3) == 0)) {
    het_set_error("%s: rows of 4 .. %d elements, a multiple of 4, %d-byte aligned, with 16-byte aligned gamma / beta only (X=%lld)", op,
                  kLnMaxX, (int)(4 * sizeof(T)), (long long)X);
    return HET_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t tile_rows = ln_tile_rows(num_rows), tiles = ln_max_tiles(num_rows, num_types);
  HET_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", op);
  HET_KTIME("HET_rows_layer_norm", s);
  HET_LN_DISPATCH(X, ln_launch_forward, (unsigned)tiles, s, offsets, (int)num_types, (int)tile_rows, y, gamma, beta, (float)eps, out, mean,
                  rstd, (idx_t)num_rows, (int)X);
  HET_LAUNCH_CHECK("HET_rows_layer_norm");
  return HET_OK;
}

template <typename T>
int rows_layer_norm_backward(const char* op, const int64_t* offsets, int64_t num_types, const T* y, const float* gamma,
                             const float* mean, const float* rstd, const T* grad_out, T* grad_y, float* grad_gamma, float* grad_beta,
                             void* workspace, int64_t workspace_bytes, int64_t num_rows, int64_t X, het_stream stream) {
  HET_REQUIRE(offsets && num_types > 0 && num_types < (1ll << 31) && num_rows >= 0 && X > 0 && grad_gamma && grad_beta, "%s: bad arguments", op);
  if (num_rows == 0) return HET_OK;  // (nothing is written: the caller's parameter gradients of an empty tensor are zeros)
  HET_REQUIRE(y && gamma && mean && rstd && grad_out, "%s: null data pointer", op);
  const int64_t need = het_rows_layer_norm_backward_workspace_bytes(num_rows, num_types, X);
  if (!(ln_shape_ok(X) && ln_rows_aligned(y, grad_out) && ln_rows_aligned((const T*)grad_y, (const T*)nullptr) &&
        aligned16(gamma, grad_gamma, grad_beta) && aligned16(workspace) && ((uintptr_t)mean & 3) == 0 && ((uintptr_t)rstd & 3) == 0)) {
    het_set_error("%s: rows of 4 .. %d elements, a multiple of 4, %d-byte aligned, with 16-byte aligned fp32 tensors only (X=%lld)", op,
                  kLnMaxX, (int)(4 * sizeof(T)), (long long)X);
    return HET_ERR_UNSUPPORTED;
  }
  HET_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes needed (het_rows_layer_norm_backward_workspace_bytes)", op,
              (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const int64_t tile_rows = ln_tile_rows(num_rows), tiles = ln_max_tiles(num_rows, num_types);
  HET_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", op);
  {
    HET_KTIME("HET_rows_layer_norm_backward", s);
    HET_LN_DISPATCH(X, ln_launch_backward, (unsigned)tiles, s, offsets, (int)num_types, (int)tile_rows, y, gamma, mean, rstd, grad_out,
                    grad_y, (float*)workspace, (idx_t)num_rows, (int)X);
    HET_LAUNCH_CHECK("HET_rows_layer_norm_backward");
  }
  {
    HET_KTIME("HET_rows_layer_norm_colsum", s);
    hipLaunchKernelGGL(HET_rows_layer_norm_colsum, dim3((unsigned)num_types, (unsigned)ceil_div64(X, 16), 2), dim3(256), 0, s, offsets,
                       (int)tile_rows, (const float*)workspace, (long)tiles, (int)X, grad_gamma, grad_beta);
    HET_LAUNCH_CHECK("HET_rows_layer_norm_colsum");
  }
  return HET_OK;
}
}  // namespace

extern "C" int het_rows_layer_norm_ok(int64_t X) { return ln_shape_ok(X) ? 1 : 0; }

extern "C" int64_t het_rows_layer_norm_backward_workspace_bytes(int64_t num_rows, int64_t num_types, int64_t X) {
  if (num_rows < 0 || num_types <= 0 || !ln_shape_ok(X)) {
    het_set_error("het_rows_layer_norm_backward_workspace_bytes: bad arguments or unsupported width (X=%lld)", (long long)X);
    return -1;
  }
  return num_rows == 0 ? 0 : ln_max_tiles(num_rows, num_types) * 2 * X * (int64_t)sizeof(float);
}

extern "C" int het_rows_layer_norm(const int64_t* offsets, int64_t num_types, const float* y, const float* gamma, const float* beta,
                                   double eps, float* out, float* mean, float* rstd, int64_t num_rows, int64_t X, het_stream stream) {
  return rows_layer_norm("het_rows_layer_norm", offsets, num_types, y, gamma, beta, eps, out, mean, rstd, num_rows, X, stream);
}

extern "C" int het_rows_layer_norm_bf16(const int64_t* offsets, int64_t num_types, const het_bf16* y, const float* gamma,
                                        const float* beta, double eps, het_bf16* out, float* mean, float* rstd, int64_t num_rows,
                                        int64_t X, het_stream stream) {
  return rows_layer_norm("het_rows_layer_norm_bf16", offsets, num_types, y, gamma, beta, eps, out, mean, rstd, num_rows, X, stream);
}

extern "C" int het_rows_layer_norm_backward(const int64_t* offsets, int64_t num_types, const float* y, const float* gamma,
                                            const float* mean, const float* rstd, const float* grad_out, float* grad_y,
                                            float* grad_gamma, float* grad_beta, void* workspace, int64_t workspace_bytes,
                                            int64_t num_rows, int64_t X, het_stream stream) {
  return rows_layer_norm_backward("het_rows_layer_norm_backward", offsets, num_types, y, gamma, mean, rstd, grad_out, grad_y, grad_gamma,
                                  grad_beta, workspace, workspace_bytes, num_rows, X, stream);
}

extern "C" int het_rows_layer_norm_backward_bf16(const int64_t* offsets, int64_t num_types, const het_bf16* y, const float* gamma,
                                                 const float* mean, const float* rstd, const het_bf16* grad_out, het_bf16* grad_y,
                                                 float* grad_gamma, float* grad_beta, void* workspace, int64_t workspace_bytes,
                                                 int64_t num_rows, int64_t X, het_stream stream) {
  return rows_layer_norm_backward("het_rows_layer_norm_backward_bf16", offsets, num_types, y, gamma, mean, rstd, grad_out, grad_y,
                                  grad_gamma, grad_beta, workspace, workspace_bytes, num_rows, X, stream);
}
