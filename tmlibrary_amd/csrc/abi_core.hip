// C-ABI of libtmhip.so (include/tmhip.h): errors, kernel timing, device and memory.
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include "abi_internal.h"

namespace tmh {

// the error channel: the calling thread's last message (guard, abi_internal.h)
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// per-kernel event timing
struct ProfSlot {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0.0;
  int64_t launches = 0;
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::map<std::string, ProfSlot> g_prof;

ProfScope::ProfScope(const char* name, hipStream_t s) : name_(name), s_(s), slot_(nullptr) {
  if (!g_prof_on) return;
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
  (void)hipEventRecord(a, s);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  auto& slot = g_prof[name];
  slot.pending.emplace_back(a, b);
  slot_ = &slot;
}

ProfScope::~ProfScope() {
  if (!slot_) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  auto* slot = static_cast<ProfSlot*>(slot_);
  (void)hipEventRecord(slot->pending.back().second, s_);
}

static void prof_drain(ProfSlot& slot) {
  for (auto& p : slot.pending) {
    float ms = 0.f;
    (void)hipEventSynchronize(p.second);
    if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) slot.total_ms += ms;
    slot.launches += 1;
    (void)hipEventDestroy(p.first);
    (void)hipEventDestroy(p.second);
  }
  slot.pending.clear();
}

// memcpy between pageable and pinned host memory, split over up to max_t
// threads (TMH_OPT_COPY_THREADS, default 8): one thread moves <= 30 GB/s and
// much less into a fresh (unfaulted) numpy output, below a PCIe 5 x16 link.
void par_copy(void* dst, const void* src, size_t bytes, int max_t) {
  const size_t min_part = (size_t)4 << 20;
  size_t nt = std::min<size_t>((size_t)std::max(1, max_t), std::max<size_t>(1, bytes / min_part));
  nt = std::min<size_t>(nt, std::max(1u, std::thread::hardware_concurrency()));
  if (nt <= 1) {
    std::memcpy(dst, src, bytes);
    return;
  }
  const size_t part = ((bytes + nt - 1) / nt + 63) & ~(size_t)63;
  std::vector<std::thread> ts;
  for (size_t i = 1; i < nt; ++i) {
    const size_t b = i * part;
    if (b >= bytes) break;
    const size_t e = std::min(bytes, b + part);
    ts.emplace_back([=] { std::memcpy((char*)dst + b, (const char*)src + b, e - b); });
  }
  std::memcpy(dst, src, std::min(bytes, part));
  for (auto& t : ts) t.join();
}

}  // namespace tmh

extern "C" {

int tmh_abi_version(void) { return TMH_ABI_VERSION; }
const char* tmh_last_error(void) { return g_last_error.c_str(); }

int tmh_device_count(int* n) {
  return guard([&] {
    TMH_CHECK(n, TMH_EINVAL, "n is NULL");
    TMH_HIP(hipGetDeviceCount(n));
  });
}

int tmh_set_device(int device) { return guard([&] { TMH_HIP(hipSetDevice(device)); }); }

int tmh_synchronize(void* stream) {
  return guard([&] {
    if (stream)
      TMH_HIP(hipStreamSynchronize((hipStream_t)stream));
    else
      TMH_HIP(hipDeviceSynchronize());
  });
}

int tmh_malloc_device(void** dev_ptr, size_t bytes) {
  return guard([&] {
    TMH_CHECK(dev_ptr, TMH_EINVAL, "dev_ptr is NULL");
    if (hipMalloc(dev_ptr, bytes) != hipSuccess) {
      *dev_ptr = nullptr;
      throw Error{TMH_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed"};
    }
  });
}

int tmh_free_device(void* dev_ptr) { return guard([&] { TMH_HIP(hipFree(dev_ptr)); }); }

int tmh_memcpy(void* dst, const void* src, size_t bytes, int kind, void* stream) {
  return guard([&] {
    TMH_CHECK(kind >= 0 && kind <= 2, TMH_EINVAL, "kind must be 0 (h2d), 1 (d2h) or 2 (d2d)");
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                          : kind == 1 ? hipMemcpyDeviceToHost
                                      : hipMemcpyDeviceToDevice;
    TMH_HIP(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
    TMH_HIP(hipStreamSynchronize((hipStream_t)stream));
  });
}

int tmh_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  return TMH_OK;
}

int tmh_profile_read(const char* kernel, double* total_ms, int64_t* launches) {
  return guard([&] {
    TMH_CHECK(kernel && total_ms && launches, TMH_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_prof.find(kernel);
    if (it == g_prof.end()) {
      *total_ms = 0.0;
      *launches = 0;
      return;
    }
    prof_drain(it->second);
    *total_ms = it->second.total_ms;
    *launches = it->second.launches;
  });
}

int tmh_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& kv : g_prof) {
    prof_drain(kv.second);
    kv.second.total_ms = 0.0;
    kv.second.launches = 0;
  }
  return TMH_OK;
}

}  // extern "C"
