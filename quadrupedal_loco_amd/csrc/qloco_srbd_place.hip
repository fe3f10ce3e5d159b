// qloco_srbd_place.hip -- the ordering kernel behind the placement state of
// the one-wave literal SRBD kernel (qloco_srbd_place.hpp):
// after a solve has left every instance's iteration count in hint[], one
// workgroup sorts the instances by class (counting sort in LDS, the longest
// class first) and writes the next call's order[]: position -> instance.
#include <vector>

#include "qloco_common.hpp"
#include "qloco_srbd_core.hpp"
#include "qloco_srbd_place.hpp"

namespace qloco {

constexpr int kPlaceThreads = 1024;

// Any contents of hint[] give a permutation: every instance takes one rank
// from its class's cursor, and place_position is a bijection.  The order
// inside a class follows the atomics and is immaterial.  The ready word is
// written last (the next solve on the stream reads it after this kernel).
__global__ __launch_bounds__(kPlaceThreads) void srbd_place_kernel(int *place, int batch, int simds,
                                                                    int check_termination) {
  __shared__ int count[kPlaceClasses];
  __shared__ int cursor[kPlaceClasses];
  const int t = threadIdx.x;
  const int *hint = place + kPlaceHeader;
  int *order = place + kPlaceHeader + batch;
  if (t < kPlaceClasses) count[t] = 0;
  __syncthreads();
  for (int i = t; i < batch; i += kPlaceThreads)
    atomicAdd(&count[place_class(hint[i], check_termination)], 1);
  __syncthreads();
  if (t < kPlaceClasses) {  // first rank of class t: the instances of the classes above it
    int first = 0;
    for (int c = t + 1; c < kPlaceClasses; ++c) first += count[c];
    cursor[t] = first;
  }
  __syncthreads();
  for (int i = t; i < batch; i += kPlaceThreads) {
    const int rank = atomicAdd(&cursor[place_class(hint[i], check_termination)], 1);
    order[place_position(rank, batch, simds)] = i;
  }
  __syncthreads();
  if (t == 0) place[0] = batch;
}

int srbd_place_launch(int32_t *place, int64_t batch, int simds, int check_termination,
                      hipStream_t stream) {
  hipLaunchKernelGGL(srbd_place_kernel, dim3(1), dim3(kPlaceThreads), 0, stream, place, (int)batch,
                     simds, check_termination);
  QLOCO_HIP_CHECK(hipGetLastError(), "srbd_place_kernel launch");
  return QLOCO_OK;
}

}  // namespace qloco

extern "C" int64_t qloco_srbd_place_bytes(int64_t batch) {
  if (batch < 0 || batch > (int64_t)1 << 30) return 0;
  return (int64_t)sizeof(int32_t) * (qloco::kPlaceHeader + 2 * batch);
}

extern "C" int qloco_srbd_place_order_host(int64_t batch, int64_t simds, int32_t check_termination,
                                           const int32_t *hint, int32_t *order) {
  using namespace qloco;
  if (!hint || !order || simds < 1 || batch <= simds || batch > 4 * simds ||
      batch > (int64_t)1 << 30)
    return QLOCO_ERR_ARG;
  std::vector<int64_t> cursor(kPlaceClasses + 1, 0);
  for (int64_t i = 0; i < batch; ++i) ++cursor[place_class(hint[i], check_termination)];
  int64_t first = 0;
  for (int c = kPlaceClasses - 1; c >= 0; --c) {
    const int64_t n = cursor[c];
    cursor[c] = first;
    first += n;
  }
  for (int64_t i = 0; i < batch; ++i) {
    const int64_t rank = cursor[place_class(hint[i], check_termination)]++;
    order[place_position(rank, batch, simds)] = (int32_t)i;
  }
  return QLOCO_OK;
}

extern "C" int qloco_srbd_place_assign_host(int64_t batch, int64_t simds,
                                            int32_t *rank_of_position) {
  using namespace qloco;
  if (!rank_of_position || simds < 1 || batch <= simds || batch > 4 * simds ||
      batch > (int64_t)1 << 30)
    return QLOCO_ERR_ARG;
  for (int64_t p = 0; p < batch; ++p) rank_of_position[p] = (int32_t)place_assign(p, batch, simds);
  return QLOCO_OK;
}
