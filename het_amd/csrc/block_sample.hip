// Keyed neighbour sampling and block construction for sampled mini-batches (het_amd/sampling.py, method="keyed").
//
// The rule (all arithmetic uint64, wrapping; pos = an edge's position in the graph's in-CSR):
//   sm(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
//   stream = sm(seed ^ sm(draw))      key(pos) = sm(stream + pos)
//   a destination of in-degree deg keeps all its in-edges when deg <= fanout or fanout <= 0, else the fanout edges with the smallest
//   (key, pos); kept edges come out in ascending pos.
// sm is a bijection of the 64-bit integers (an addition and two xor-shift / odd-multiply rounds), so the keys of one stream are
// distinct and the (key, pos) order never reaches its second component; the selection below honours it all the same.
//
//   het_sample_count            kept edges per destination, exclusive scan (hipCUB), total to the host
//   het_sample_select           pos / owner of the kept edges: keys are recomputed from pos, no edge array is read
//   het_block_renumber          local ids: destinations first, then the new sources sorted by global id
//   het_block_relation_major    stable sort by relation: rel_ptrs, row, col, rel_types, global edge ids in block order
//
// Selection is exact: the fanout-th smallest key P of a row is found most significant digit first, then every edge with key < P
// (and the first few with key == P, by pos) is emitted at offsets[b] + its rank among the kept ones, by ballot and prefix counts.
//   deg <  kSampleWorkgroupDegree: one wave per destination, the row's keys in registers (kSampleWaveItems per lane), P bit by bit
//                                  with one ballot per (bit, item): no LDS, no barrier.
//   deg >= kSampleWorkgroupDegree: one workgroup of kSampleChunk threads per destination, P in 8 passes of 8 bits (a 256-bin LDS
//                                  histogram of the keys that match the digits found so far), emission in chunks of kSampleChunk
//                                  positions.  In-degrees below 2^32.
// All stores are ordinary vector stores; the atomics are LDS adds (histogram) and global compare-and-swap / add (renumbering).
#include <hipcub/hipcub.hpp>

#include "common.hip.h"  // (sm64)
#include "device_scratch.hip.h"

namespace {

constexpr int kSampleWorkgroupDegree = 512;                        // in-degree from which a workgroup takes the destination
constexpr int kSampleWaveItems = kSampleWorkgroupDegree / HET_WAVE;  // keys per lane on the wave path
constexpr int kSampleChunk = 1024;                                 // threads of the long-row workgroup = positions per emission chunk
constexpr int kSampleChunkWaves = kSampleChunk / HET_WAVE;

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// (start, degree) of destination b; a destination outside [0, N) has no edges
__device__ __forceinline__ void dst_row(const idx_t* __restrict__ row_ptrs, const idx_t* __restrict__ dst, idx_t b, idx_t N,
                                        idx_t& start, idx_t& deg) {
  const idx_t v = dst[b];
  start = 0;
  deg = 0;
  if ((uint64_t)v < (uint64_t)N) {
    start = row_ptrs[v];
    deg = row_ptrs[v + 1] - start;
    if (deg < 0) deg = 0;
  }
}

__global__ void HET_sample_count(const idx_t* __restrict__ row_ptrs, const idx_t* __restrict__ dst, idx_t B, idx_t N, idx_t fanout,
                                 idx_t* __restrict__ counts) {
  for (idx_t b = (idx_t)blockIdx.x * kBlock + threadIdx.x; b <= B; b += (idx_t)gridDim.x * kBlock) {
    idx_t start, deg = 0;
    if (b < B) dst_row(row_ptrs, dst, b, N, start, deg);
    counts[b] = (fanout > 0 && deg > fanout) ? fanout : deg;  // (counts[B] = 0: the scan's last output is the total)
  }
}

// One wave per destination of in-degree below kSampleWorkgroupDegree.
__global__ __launch_bounds__(kBlock) void HET_sample_select_wave(const idx_t* __restrict__ row_ptrs, const idx_t* __restrict__ dst,
                                                                 idx_t B, idx_t N, idx_t fanout, uint64_t stream,
                                                                 const idx_t* __restrict__ offsets, idx_t total,
                                                                 idx_t* __restrict__ out_pos, idx_t* __restrict__ out_owner) {
  const int lane = threadIdx.x % HET_WAVE;
  const uint64_t below = lanes_below(lane);
  const idx_t waves = (idx_t)gridDim.x * (kBlock / HET_WAVE);
  for (idx_t b = (idx_t)blockIdx.x * (kBlock / HET_WAVE) + threadIdx.x / HET_WAVE; b < B; b += waves) {
    idx_t start, deg;
    dst_row(row_ptrs, dst, b, N, start, deg);
    if (deg == 0 || deg >= kSampleWorkgroupDegree) continue;
    const idx_t out = offsets[b];
    if (fanout <= 0 || deg <= fanout) {  // keeps everything: a straight copy
      if (out + deg > total) continue;   // (offsets that do not belong to this call: nothing is written)
      for (idx_t j = lane; j < deg; j += HET_WAVE) {
        out_pos[out + j] = start + j;
        out_owner[out + j] = b;
      }
      continue;
    }
    if (out + fanout > total) continue;
    const int items = (int)((deg + HET_WAVE - 1) / HET_WAVE);
    uint64_t key[kSampleWaveItems];
    bool valid[kSampleWaveItems];
#pragma unroll
    for (int i = 0; i < kSampleWaveItems; ++i) {
      const idx_t j = (idx_t)i * HET_WAVE + lane;
      valid[i] = i < items && j < deg;
      key[i] = valid[i] ? sm64(stream + (uint64_t)(start + j)) : 0ull;
    }
    // P = the fanout-th smallest key, most significant bit first: `k` of the keys that agree with P on the decided bits are wanted
    uint64_t P = 0, decided = 0;
    idx_t k = fanout;
    for (int bit = 63; bit >= 0; --bit) {
      const uint64_t m = 1ull << bit;
      idx_t zeros = 0;
#pragma unroll
      for (int i = 0; i < kSampleWaveItems; ++i)
        if (i < items) zeros += __popcll(__ballot(valid[i] && (key[i] & decided) == P && !(key[i] & m)));
      if (k > zeros) {
        P |= m;
        k -= zeros;
      }
      decided |= m;
    }
    // now k = how many of the keys equal to P are kept (the first k by pos)
    idx_t less_base = 0, eq_base = 0;
#pragma unroll
    for (int i = 0; i < kSampleWaveItems; ++i) {
      if (i < items) {
        const bool less = valid[i] && key[i] < P, eq = valid[i] && key[i] == P;
        const uint64_t bl = __ballot(less), be = __ballot(eq);
        const idx_t lb = less_base + __popcll(bl & below), eb = eq_base + __popcll(be & below);
        if (less || (eq && eb < k)) {
          const idx_t at = lb + (eb < k ? eb : k);  // rank among the kept edges: below fanout by construction
          if (at < fanout) {
            out_pos[out + at] = start + (idx_t)i * HET_WAVE + lane;
            out_owner[out + at] = b;
          }
        }
        less_base += __popcll(bl);
        eq_base += __popcll(be);
      }
    }
  }
}

// One workgroup per destination of in-degree kSampleWorkgroupDegree or more (the others are skipped: the branch is uniform).
__global__ __launch_bounds__(kSampleChunk) void HET_sample_select_group(const idx_t* __restrict__ row_ptrs,
                                                                        const idx_t* __restrict__ dst, idx_t B, idx_t N, idx_t fanout,
                                                                        uint64_t stream, const idx_t* __restrict__ offsets, idx_t total,
                                                                        idx_t* __restrict__ out_pos, idx_t* __restrict__ out_owner) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wave_less[kSampleChunkWaves], wave_eq[kSampleChunkWaves];
  __shared__ unsigned s_digit;
  __shared__ idx_t s_k;
  const int tid = threadIdx.x, lane = tid % HET_WAVE, wave = tid / HET_WAVE;
  const uint64_t below = lanes_below(lane);
  for (idx_t b = blockIdx.x; b < B; b += gridDim.x) {
    idx_t start, deg;
    dst_row(row_ptrs, dst, b, N, start, deg);
    if (deg < kSampleWorkgroupDegree) continue;
    const idx_t out = offsets[b];
    if (fanout <= 0 || deg <= fanout) {
      if (out + deg > total) continue;
      for (idx_t j = tid; j < deg; j += kSampleChunk) {
        out_pos[out + j] = start + j;
        out_owner[out + j] = b;
      }
      continue;
    }
    if (out + fanout > total) continue;
    uint64_t P = 0, decided = 0;
    idx_t k = fanout;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (idx_t j = tid; j < deg; j += kSampleChunk) {
        const uint64_t key = sm64(stream + (uint64_t)(start + j));
        if ((key & decided) == P) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < HET_WAVE) {  // the first wave finds the digit whose bin holds the k-th key: lane l owns bins 4l .. 4l+3
        unsigned c[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          c[q] = hist[4 * tid + q];
          sum += c[q];
        }
        unsigned incl = sum;
        for (int d = 1; d < HET_WAVE; d <<= 1) {
          const unsigned t = __shfl_up(incl, d);
          if (lane >= d) incl += t;
        }
        idx_t before = (idx_t)incl - (idx_t)sum;
        if (before < k && k <= (idx_t)incl) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (k > before && k <= before + (idx_t)c[q]) {
              s_digit = 4 * tid + q;
              s_k = k - before;
            }
            before += c[q];
          }
        }
      }
      __syncthreads();
      P |= (uint64_t)s_digit << shift;
      decided |= 0xffull << shift;
      k = s_k;
    }
    idx_t less_base = 0, eq_base = 0;
    for (idx_t c0 = 0; c0 < deg; c0 += kSampleChunk) {
      const idx_t j = c0 + tid;
      const bool valid = j < deg;
      const uint64_t key = valid ? sm64(stream + (uint64_t)(start + j)) : 0ull;
      const bool less = valid && key < P, eq = valid && key == P;
      const uint64_t bl = __ballot(less), be = __ballot(eq);
      if (lane == 0) {
        wave_less[wave] = __popcll(bl);
        wave_eq[wave] = __popcll(be);
      }
      __syncthreads();
      idx_t lb = less_base + __popcll(bl & below), eb = eq_base + __popcll(be & below);
      unsigned tl = 0, te = 0;
#pragma unroll
      for (int q = 0; q < kSampleChunkWaves; ++q) {
        const unsigned a = wave_less[q], e = wave_eq[q];
        if (q < wave) {
          lb += a;
          eb += e;
        }
        tl += a;
        te += e;
      }
      if (less || (eq && eb < k)) {
        const idx_t at = lb + (eb < k ? eb : k);
        if (at < fanout) {
          out_pos[out + at] = start + j;
          out_owner[out + at] = b;
        }
      }
      less_base += tl;
      eq_base += te;
      __syncthreads();  // (the wave counts are rewritten by the next chunk)
    }
  }
}

// nodes[b] = dst[b], map[dst[b]] = b
__global__ void HET_block_mark_dst(const idx_t* __restrict__ dst, idx_t B, idx_t N, idx_t* __restrict__ map, idx_t* __restrict__ nodes) {
  for (idx_t b = (idx_t)blockIdx.x * kBlock + threadIdx.x; b < B; b += (idx_t)gridDim.x * kBlock) {
    const idx_t v = dst[b];
    nodes[b] = v;
    if ((uint64_t)v < (uint64_t)N) map[v] = b;
  }
}

__device__ __forceinline__ idx_t sampled_source(const idx_t* __restrict__ src, const idx_t* __restrict__ pos, idx_t e, idx_t E, idx_t N) {
  const idx_t p = pos[e];
  if ((uint64_t)p >= (uint64_t)E) return -1;
  const idx_t s = src[p];
  return (uint64_t)s < (uint64_t)N ? s : -1;
}

// Every sampled source that is no destination (map == -1) is claimed exactly once (compare-and-swap -1 -> -2) and appended to
// `list`: one add of the wave's count to the list's counter, the wave's claimers at consecutive places after it.  Which lane wins
// a node and where it lands in the list depends on the order the atomics land in; the list is sorted by global id before any id
// is assigned, so nothing downstream does.
__global__ void HET_block_claim(const idx_t* __restrict__ src, const idx_t* __restrict__ pos, idx_t total, idx_t E, idx_t N,
                                idx_t* __restrict__ map, idx_t* __restrict__ list, unsigned long long* __restrict__ counter) {
  const int lane = threadIdx.x % HET_WAVE;
  for (idx_t base = (idx_t)blockIdx.x * kBlock; base < total; base += (idx_t)gridDim.x * kBlock) {
    const idx_t e = base + threadIdx.x;
    idx_t s = -1;
    bool claimed = false;
    if (e < total) {
      s = sampled_source(src, pos, e, E, N);
      if (s >= 0 && map[s] == -1)
        claimed = atomicCAS(reinterpret_cast<unsigned long long*>(map + s), (unsigned long long)-1ll, (unsigned long long)-2ll) ==
                  (unsigned long long)-1ll;
    }
    const uint64_t won = __ballot(claimed);
    if (won) {
      const int leader = __ffsll((unsigned long long)won) - 1;
      unsigned long long at = 0;
      if (lane == leader) at = atomicAdd(counter, (unsigned long long)__popcll(won));
      at = __shfl(at, leader);
      if (claimed) list[at + __popcll(won & lanes_below(lane))] = s;
    }
  }
}

// map[extra[i]] = B + i (extra = nodes + B, sorted by global id)
__global__ void HET_block_assign(const idx_t* __restrict__ extra, idx_t n, idx_t B, idx_t N, idx_t* __restrict__ map) {
  for (idx_t i = (idx_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (idx_t)gridDim.x * kBlock) {
    const idx_t v = extra[i];
    if ((uint64_t)v < (uint64_t)N) map[v] = B + i;
  }
}

__global__ void HET_block_local_src(const idx_t* __restrict__ src, const idx_t* __restrict__ pos, idx_t total, idx_t E, idx_t N,
                                    const idx_t* __restrict__ map, idx_t* __restrict__ local_src) {
  for (idx_t e = (idx_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (idx_t)gridDim.x * kBlock) {
    const idx_t s = sampled_source(src, pos, e, E, N);
    local_src[e] = s >= 0 ? map[s] : -1;
  }
}

__global__ void HET_block_restore(const idx_t* __restrict__ nodes, idx_t n, idx_t N, idx_t* __restrict__ map) {
  for (idx_t i = (idx_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (idx_t)gridDim.x * kBlock) {
    const idx_t v = nodes[i];
    if ((uint64_t)v < (uint64_t)N) map[v] = -1;
  }
}

__global__ void HET_block_rel_keys(const idx_t* __restrict__ rel, const idx_t* __restrict__ pos, idx_t total, idx_t E, idx_t R,
                                   uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  for (idx_t e = (idx_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (idx_t)gridDim.x * kBlock) {
    const idx_t p = pos[e];
    const idx_t r = (uint64_t)p < (uint64_t)E ? rel[p] : 0;
    keys[e] = (uint64_t)r < (uint64_t)R ? (uint32_t)r : (uint32_t)(R - 1);  // (a relation outside [0, R) cannot widen the sort)
    vals[e] = (int32_t)e;
  }
}

// block order j <- sampled order perm[j]; the first R + 1 threads also place the relation pointers by binary search
__global__ void HET_block_rel_gather(const uint32_t* __restrict__ sorted, const int32_t* __restrict__ perm, idx_t total, idx_t E, idx_t R,
                                     const idx_t* __restrict__ eids, const idx_t* __restrict__ pos, const idx_t* __restrict__ owner,
                                     const idx_t* __restrict__ local_src, idx_t* __restrict__ out_rel_ptrs, idx_t* __restrict__ out_row,
                                     idx_t* __restrict__ out_col, idx_t* __restrict__ out_rel, idx_t* __restrict__ out_eids) {
  const idx_t n = total > R + 1 ? total : R + 1;
  for (idx_t j = (idx_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (idx_t)gridDim.x * kBlock) {
    if (j < total) {
      const idx_t e = perm[j];
      const idx_t p = pos[e];
      out_row[j] = local_src[e];
      out_col[j] = owner[e];
      out_rel[j] = sorted[j];
      out_eids[j] = (uint64_t)p < (uint64_t)E ? eids[p] : -1;
    }
    if (j <= R) {  // number of edges with relation < j
      idx_t lo = 0, hi = total;
      while (lo < hi) {
        const idx_t mid = (lo + hi) >> 1;
        if ((idx_t)sorted[mid] < j) lo = mid + 1; else hi = mid;
      }
      out_rel_ptrs[j] = lo;
    }
  }
}

constexpr int64_t kMaxBlockEdges = 1ll << 30;  // block positions are sorted as int32 values

}  // namespace

extern "C" int het_sample_workgroup_degree(void) { return kSampleWorkgroupDegree; }
extern "C" int het_sample_chunk(void) { return kSampleChunk; }

extern "C" int het_sample_count(const int64_t* row_ptrs, const int64_t* dst, int64_t num_dst, int64_t num_nodes, int64_t fanout,
                                int64_t* out_offsets, int64_t* out_total, het_stream stream) {
  const char* op = "het_sample_count";
  HET_REQUIRE(num_dst >= 0 && num_nodes >= 0 && num_dst < (1ll << 31) - 1, "%s: bad arguments (num_dst=%lld, num_nodes=%lld)", op,
              (long long)num_dst, (long long)num_nodes);
  if (out_total) *out_total = 0;
  if (num_dst == 0) return HET_OK;
  HET_REQUIRE(row_ptrs && dst && out_offsets && out_total, "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  Scratch tmp(s);
  idx_t* counts = nullptr;
  HET_HIP(tmp.alloc((void**)&counts, sizeof(idx_t) * (num_dst + 1)));
  {
    HET_KTIME("HET_sample_count", s);
    hipLaunchKernelGGL(HET_sample_count, dim3(grid_for(num_dst + 1)), dim3(kBlock), 0, s, row_ptrs, dst, (idx_t)num_dst, (idx_t)num_nodes,
                       (idx_t)fanout, counts);
  }
  HET_LAUNCH_CHECK("HET_sample_count");
  size_t tb = 0;
  HET_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, counts, out_offsets, (int)(num_dst + 1), s));
  void* t0 = nullptr;
  HET_HIP(tmp.alloc((void**)&t0, tb));
  HET_HIP(hipcub::DeviceScan::ExclusiveSum(t0, tb, counts, out_offsets, (int)(num_dst + 1), s));
  int64_t h_total = 0;
  HET_HIP(hipMemcpyAsync(&h_total, out_offsets + num_dst, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HET_HIP(hipStreamSynchronize(s));
  *out_total = h_total;
  return HET_OK;
}

extern "C" int het_sample_select(const int64_t* row_ptrs, const int64_t* dst, int64_t num_dst, int64_t num_nodes, int64_t fanout,
                                 int64_t seed, int64_t draw, const int64_t* offsets, int64_t total, int64_t* out_pos,
                                 int64_t* out_owner, het_stream stream) {
  const char* op = "het_sample_select";
  HET_REQUIRE(num_dst >= 0 && num_nodes >= 0 && total >= 0, "%s: bad arguments (num_dst=%lld, num_nodes=%lld, total=%lld)", op,
              (long long)num_dst, (long long)num_nodes, (long long)total);
  if (num_dst == 0 || total == 0) return HET_OK;
  HET_REQUIRE(row_ptrs && dst && offsets && out_pos && out_owner, "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t key_stream = sm64((uint64_t)seed ^ sm64((uint64_t)draw));
  {
    HET_KTIME("HET_sample_select_wave", s);
    hipLaunchKernelGGL(HET_sample_select_wave, dim3(grid_for(num_dst * HET_WAVE)), dim3(kBlock), 0, s, row_ptrs, dst, (idx_t)num_dst,
                       (idx_t)num_nodes, (idx_t)fanout, key_stream, offsets, (idx_t)total, out_pos, out_owner);
  }
  HET_LAUNCH_CHECK("HET_sample_select_wave");
  {
    HET_KTIME("HET_sample_select_group", s);
    const unsigned groups = (unsigned)(num_dst < 2048 ? num_dst : 2048);
    hipLaunchKernelGGL(HET_sample_select_group, dim3(groups), dim3(kSampleChunk), 0, s, row_ptrs, dst, (idx_t)num_dst, (idx_t)num_nodes,
                       (idx_t)fanout, key_stream, offsets, (idx_t)total, out_pos, out_owner);
  }
  HET_LAUNCH_CHECK("HET_sample_select_group");
  return HET_OK;
}

extern "C" int het_block_renumber(const int64_t* src, int64_t num_edges, const int64_t* pos, int64_t total, const int64_t* dst,
                                  int64_t num_dst, int64_t* map, int64_t num_nodes, int64_t* out_nodes, int64_t* out_local_src,
                                  int64_t* out_num_extra, het_stream stream) {
  const char* op = "het_block_renumber";
  HET_REQUIRE(num_edges >= 0 && total >= 0 && num_dst >= 0 && num_nodes >= 0 && total < kMaxBlockEdges,
              "%s: bad arguments (num_edges=%lld, total=%lld, num_dst=%lld, num_nodes=%lld)", op, (long long)num_edges, (long long)total,
              (long long)num_dst, (long long)num_nodes);
  if (out_num_extra) *out_num_extra = 0;
  if (num_dst == 0 || total == 0) return HET_OK;
  HET_REQUIRE(src && pos && dst && map && out_nodes && out_local_src && out_num_extra, "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  Scratch tmp(s);
  idx_t* list = nullptr;
  unsigned long long* counter = nullptr;
  HET_HIP(tmp.alloc((void**)&list, sizeof(idx_t) * total));
  HET_HIP(tmp.alloc((void**)&counter, sizeof(unsigned long long)));
  HET_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), s));
  HET_KTIME("HET_block_renumber", s);
  hipLaunchKernelGGL(HET_block_mark_dst, dim3(grid_for(num_dst)), dim3(kBlock), 0, s, dst, (idx_t)num_dst, (idx_t)num_nodes, map, out_nodes);
  HET_LAUNCH_CHECK("HET_block_mark_dst");
  hipLaunchKernelGGL(HET_block_claim, dim3(grid_for(total)), dim3(kBlock), 0, s, src, pos, (idx_t)total, (idx_t)num_edges,
                     (idx_t)num_nodes, map, list, counter);
  HET_LAUNCH_CHECK("HET_block_claim");
  unsigned long long h_extra = 0;
  HET_HIP(hipMemcpyAsync(&h_extra, counter, sizeof(h_extra), hipMemcpyDeviceToHost, s));
  HET_HIP(hipStreamSynchronize(s));
  const int64_t extra = (int64_t)h_extra;
  if (extra > total) {  // (cannot happen: every claim is one of `total` lanes)
    het_set_error("%s: %lld new nodes claimed by %lld edges", op, (long long)extra, (long long)total);
    return HET_ERR_HIP;
  }
  if (extra > 0) {
    // ascending global id: the local ids B + i do not depend on the order in which the claims landed
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(list);
    uint64_t* keys_out = reinterpret_cast<uint64_t*>(out_nodes + num_dst);
    const int bits = bits_for(num_nodes);
    size_t tb = 0;
    HET_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, keys_in, keys_out, (int)extra, 0, bits, s));
    void* t0 = nullptr;
    HET_HIP(tmp.alloc((void**)&t0, tb));
    HET_HIP(hipcub::DeviceRadixSort::SortKeys(t0, tb, keys_in, keys_out, (int)extra, 0, bits, s));
    hipLaunchKernelGGL(HET_block_assign, dim3(grid_for(extra)), dim3(kBlock), 0, s, out_nodes + num_dst, (idx_t)extra, (idx_t)num_dst,
                       (idx_t)num_nodes, map);
    HET_LAUNCH_CHECK("HET_block_assign");
  }
  hipLaunchKernelGGL(HET_block_local_src, dim3(grid_for(total)), dim3(kBlock), 0, s, src, pos, (idx_t)total, (idx_t)num_edges,
                     (idx_t)num_nodes, map, out_local_src);
  HET_LAUNCH_CHECK("HET_block_local_src");
  hipLaunchKernelGGL(HET_block_restore, dim3(grid_for(num_dst + extra)), dim3(kBlock), 0, s, out_nodes, (idx_t)(num_dst + extra),
                     (idx_t)num_nodes, map);
  HET_LAUNCH_CHECK("HET_block_restore");
  *out_num_extra = extra;
  return HET_OK;
}

extern "C" int het_block_relation_major(const int64_t* rel, const int64_t* eids, int64_t num_edges, const int64_t* pos,
                                        const int64_t* owner, const int64_t* local_src, int64_t total, int64_t num_rels,
                                        int64_t* out_rel_ptrs, int64_t* out_row, int64_t* out_col, int64_t* out_rel, int64_t* out_eids,
                                        het_stream stream) {
  const char* op = "het_block_relation_major";
  HET_REQUIRE(num_edges >= 0 && total >= 0 && total < kMaxBlockEdges, "%s: bad arguments (num_edges=%lld, total=%lld)", op,
              (long long)num_edges, (long long)total);
  HET_REQUIRE(num_rels >= 1 && num_rels < (1ll << 31), "%s: num_rels=%lld (at least one relation expected)", op, (long long)num_rels);
  if (total == 0) return HET_OK;
  HET_REQUIRE(rel && eids && pos && owner && local_src && out_rel_ptrs && out_row && out_col && out_rel && out_eids, "%s: null pointer", op);
  hipStream_t s = (hipStream_t)stream;
  Scratch tmp(s);
  uint32_t *keys_in = nullptr, *keys_out = nullptr;
  int32_t *vals_in = nullptr, *perm = nullptr;
  HET_HIP(tmp.alloc((void**)&keys_in, sizeof(uint32_t) * total));
  HET_HIP(tmp.alloc((void**)&keys_out, sizeof(uint32_t) * total));
  HET_HIP(tmp.alloc((void**)&vals_in, sizeof(int32_t) * total));
  HET_HIP(tmp.alloc((void**)&perm, sizeof(int32_t) * total));
  HET_KTIME("HET_block_relation_major", s);
  hipLaunchKernelGGL(HET_block_rel_keys, dim3(grid_for(total)), dim3(kBlock), 0, s, rel, pos, (idx_t)total, (idx_t)num_edges,
                     (idx_t)num_rels, keys_in, vals_in);
  HET_LAUNCH_CHECK("HET_block_rel_keys");
  const int bits = bits_for(num_rels);
  size_t tb = 0;
  HET_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in, keys_out, vals_in, perm, (int)total, 0, bits, s));
  void* t0 = nullptr;
  HET_HIP(tmp.alloc((void**)&t0, tb));
  HET_HIP(hipcub::DeviceRadixSort::SortPairs(t0, tb, keys_in, keys_out, vals_in, perm, (int)total, 0, bits, s));
  const int64_t n = total > num_rels + 1 ? total : num_rels + 1;
  hipLaunchKernelGGL(HET_block_rel_gather, dim3(grid_for(n)), dim3(kBlock), 0, s, keys_out, perm, (idx_t)total, (idx_t)num_edges,
                     (idx_t)num_rels, eids, pos, owner, local_src, out_rel_ptrs, out_row, out_col, out_rel, out_eids);
  HET_LAUNCH_CHECK("HET_block_rel_gather");
  return HET_OK;
}
