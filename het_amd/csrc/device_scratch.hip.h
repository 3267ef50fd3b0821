// Host-side helpers of the units that sort with hipCUB (layouts.hip, block_sample.hip): the device temporaries of one entry call and
// the bit count of a radix sort's keys.
#pragma once
#include "common.hip.h"

namespace {

inline int bits_for(int64_t n) {  // bits to represent values in [0, n)
  int b = 1;
  while (b < 62 && (1ll << b) < n) ++b;
  return b;
}

struct Scratch {  // frees device temporaries on every exit path
  void* p[12] = {};
  int n = 0;
  hipStream_t s = nullptr;  // the stream the temporaries are used on (a caller's allocator orders their reuse on it)
  explicit Scratch(hipStream_t st) : s(st) {}
  ~Scratch() { for (int i = 0; i < n; ++i) (void)het_free_e(p[i]); }
  hipError_t alloc(void** out, size_t bytes) {
    hipError_t e = het_malloc_e(out, bytes ? bytes : 8, s);
    if (e == hipSuccess) p[n++] = *out;
    return e;
  }
};

}  // namespace
