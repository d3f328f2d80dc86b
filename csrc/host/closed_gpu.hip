// Host side of the closed / maximal flag kernel for a host trie (kernels: csrc/kernels/closed.hip;
// CPU twin: closed_cpu.cpp; the device-resident deep trie: GpuMiner::deep_trie_flags).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../kernels/kernels.hpp"
#include "kmls/gpu.hpp"
#include "kmls/trace.hpp"

#define KMLS_HIP(expr)                                                                  \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) +      \
                               " at " + __FILE__ + ":" + std::to_string(__LINE__));     \
  } while (0)

namespace kmls {
namespace gpu {

namespace {
struct DevBuf {  // RAII hipMalloc
  void* p = nullptr;
  explicit DevBuf(size_t bytes) { KMLS_HIP(hipMalloc(&p, std::max<size_t>(bytes, 256))); }
  ~DevBuf() { if (p) (void)hipFree(p); }
  template <class T> T* as() const { return (T*)p; }
};
}  // namespace

namespace {

// upload, one hash build, marks (with generators: three bits, and closure ids when closure_out),
// fold and resolve; the flag bytes and the closure ids come back
void flags_gpu(int device, const int64_t* parent, const int32_t* item, const uint32_t* count,
               const uint8_t* depth, int64_t n, uint8_t* flags_out, bool generators,
               int32_t* closure_out, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  if (n == 0) return;
  KMLS_CHECK(n < (1ll << 31) - 1, "GPU itemset flags: trie larger than 2^31 nodes");
  // the kernel chases parent ids: they must stay inside the arrays
  validate_trie_shape(parent, depth, n, "GPU itemset flags");
  KMLS_HIP(hipSetDevice(device));
  hipStream_t s;
  KMLS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{s};
  DevBuf d_par(n * 8), d_item(n * 4), d_cnt(n * 4), d_dep(n);
  KMLS_HIP(hipMemcpyAsync(d_par.p, parent, n * 8, hipMemcpyHostToDevice, s));
  KMLS_HIP(hipMemcpyAsync(d_item.p, item, n * 4, hipMemcpyHostToDevice, s));
  KMLS_HIP(hipMemcpyAsync(d_cnt.p, count, n * 4, hipMemcpyHostToDevice, s));
  KMLS_HIP(hipMemcpyAsync(d_dep.p, depth, n, hipMemcpyHostToDevice, s));
  const uint64_t cap = kern::closed_hash_slots(n);
  DevBuf d_keys(cap * 8), d_vals(cap * 4), d_flags(n), d_eq(n), d_err(256);
  DevBuf d_gen(generators ? n : 0), d_up(closure_out ? n * 4 : 0);
  hipDeviceProp_t prop;
  KMLS_HIP(hipGetDeviceProperties(&prop, device));
  hipEvent_t e0, e1;
  KMLS_HIP(hipEventCreate(&e0));
  KMLS_HIP(hipEventCreate(&e1));
  struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } eg{e0, e1};
  kern::ClosedScratch x{d_keys.as<unsigned long long>(), d_vals.as<int32_t>(), cap - 1,
                        d_flags.as<unsigned char>(), d_eq.as<unsigned char>(),
                        d_err.as<unsigned int>()};
  if (generators) x.gen = d_gen.as<unsigned char>();
  if (closure_out) x.up = d_up.as<unsigned int>();
  KMLS_HIP(hipEventRecord(e0, s));
  kern::closed_flags(d_par.as<int64_t>(), d_item.as<int32_t>(), d_cnt.as<uint32_t>(),
                     d_dep.as<unsigned char>(), n, x, std::max(1, prop.multiProcessorCount), s);
  KMLS_HIP(hipEventRecord(e1, s));
  unsigned int err = 0;
  KMLS_HIP(hipMemcpyAsync(&err, x.error, 4, hipMemcpyDeviceToHost, s));
  KMLS_HIP(hipMemcpyAsync(flags_out, x.flags, (size_t)n, hipMemcpyDeviceToHost, s));
  if (closure_out)
    KMLS_HIP(hipMemcpyAsync(closure_out, x.up, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  KMLS_HIP(hipStreamSynchronize(s));
  KMLS_CHECK(err == 0, "GPU itemset flags: a subset of a frequent itemset is missing from the trie "
                       "(trie not closed under subsets, or itemset longer than 63)");
  if (kernel_ms) {
    float ms = 0.f;
    KMLS_HIP(hipEventElapsedTime(&ms, e0, e1));
    *kernel_ms = ms;
  }
}

}  // namespace

void itemset_flags_gpu(int device, const int64_t* parent, const int32_t* item,
                       const uint32_t* count, const uint8_t* depth, int64_t n, uint8_t* flags_out,
                       double* kernel_ms) {
  trace::Range rg_("kmls.itemset_flags_gpu");
  flags_gpu(device, parent, item, count, depth, n, flags_out, false, nullptr, kernel_ms);
}

void itemset_condense_gpu(int device, const int64_t* parent, const int32_t* item,
                          const uint32_t* count, const uint8_t* depth, int64_t n,
                          uint8_t* flags_out, int32_t* closure_out, double* kernel_ms) {
  trace::Range rg_("kmls.itemset_condense_gpu");
  flags_gpu(device, parent, item, count, depth, n, flags_out, true, closure_out, kernel_ms);
}

}  // namespace gpu
}  // namespace kmls
