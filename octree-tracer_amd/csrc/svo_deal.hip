// svo_deal.hip -- the kernels of a resting view's static deal: svo_deal.h's seed, step and compare, each run by
// one workgroup on the context's stream (the step: by one per list).  They run on learning frames and after a rebuild of the lists only; a resting frame
// launches none of them.
#include <hip/hip_runtime.h>

#include "svo_deal.h"
#include "svo_device.h"

namespace svo {

static_assert(kDealBalStart == kBalanceStart && kDealBalStamps == kBalanceStamps && kDealBalBestTime == kBalanceBestTime &&
                  kDealBalHead == kBalanceHead && kDealBalSlots == kBalanceSlots,
              "svo_deal.h reads the balance words by svo_device.h's numbers");

constexpr uint32_t kDealThreads = 1024;

struct BlockSync {
    __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(kDealThreads) void deal_seed_kernel(Deal d, const uint32_t *order, const uint32_t *bal) {
    __shared__ uint32_t red[kDealThreads];
    deal_seed(d, order, bal, red, threadIdx.x, kDealThreads, BlockSync{});
}

__global__ __launch_bounds__(kDealThreads) void deal_compare_kernel(Deal d, const uint32_t *order) {
    __shared__ uint32_t flag;
    deal_reseed_if_changed(d, order, &flag, threadIdx.x, kDealThreads, BlockSync{});
}

// (a step is two launches: no workgroup of the first writes the state words that the others read)
__global__ __launch_bounds__(kDealThreads) void deal_step_kernel(Deal d, const uint32_t *bal) {
    __shared__ uint32_t scratch[2 * kDealMaxListWaves + kDealThreads];
    deal_step(d, bal, scratch, blockIdx.x, threadIdx.x, kDealThreads, BlockSync{});
}

__global__ __launch_bounds__(64) void deal_commit_kernel(Deal d, const uint32_t *bal) {
    if (threadIdx.x == 0u) deal_commit(d, bal);
}

hipError_t launch_deal_seed(const Deal &d, const uint32_t *order, const uint32_t *bal, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(deal_seed_kernel, dim3(1), dim3(kDealThreads), 0, stream, d, order, bal);
    return hipGetLastError();
}

hipError_t launch_deal_compare(const Deal &d, const uint32_t *order, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(deal_compare_kernel, dim3(1), dim3(kDealThreads), 0, stream, d, order);
    return hipGetLastError();
}

hipError_t launch_deal_step(const Deal &d, const uint32_t *bal, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(deal_step_kernel, dim3(8), dim3(kDealThreads), 0, stream, d, bal);
    hipLaunchKernelGGL(deal_commit_kernel, dim3(1), dim3(64), 0, stream, d, bal);
    return hipGetLastError();
}

}  // namespace svo
