// Folds of a block's sums and item counts into a call's running totals (CutoffTotals, evaluator.hip).
// (Included by evaluator.hip last of its kernel headers and in an unnamed namespace, where these two kernels have
// always stood: their symbols and their place in the code object stay what they were.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// Metrics::merge (evaluator.cpp:76-85: plain sums) on the device, one thread, and the item histogram beside it:
// a call that walks its users in blocks folds each block's result here instead of reading it back
__global__ void metrics_fold_kernel(const irs_metrics *__restrict__ part, irs_metrics *__restrict__ into) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  into->valid_user += part->valid_user;
  into->total_user += part->total_user;
  into->hit += part->hit;
  into->recall += part->recall;
  into->ndcg += part->ndcg;
  into->precision += part->precision;
  into->map += part->map;
}
__global__ void counts_fold_kernel(const unsigned long long *__restrict__ part, int64_t n,
                                   unsigned long long *__restrict__ into) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) into[i] += part[i];
}

}  // namespace
