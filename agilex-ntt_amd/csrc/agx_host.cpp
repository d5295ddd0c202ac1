// agx_host.cpp -- the entry points that work on host memory: the streaming pipeline behind agx_ntt_*_host_stream (pinned staging,
// three streams), the one-shot agx_ntt_forward_host with its cached plans, and the prime / root / table helpers.  Plans are used only
// through the public device calls.
#include "../../include/agx_ntt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "host_math.hpp"
#include "plan_internal.hpp"

using namespace agx;

namespace agx {
hipError_t staging_set::ensure(size_t want) {
    if (bytes >= want) return hipSuccess;
    destroy();
    hipError_t e = hipSuccess;
    for (int k = 0; k < kSlots && e == hipSuccess; ++k) {
        e = hipHostMalloc(reinterpret_cast<void**>(&pin_in[k]), want, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&pin_out[k]), want, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dev[k]), want);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
    }
    if (e == hipSuccess) bytes = want;
    else destroy();
    return e;
}
void staging_set::destroy() {
    for (int k = 0; k < kSlots; ++k) {
        if (st[k]) { (void)hipStreamSynchronize(st[k]); (void)hipStreamDestroy(st[k]); }
        if (done[k]) (void)hipEventDestroy(done[k]);
        if (dev[k]) (void)hipFree(dev[k]);
        if (pin_in[k]) (void)hipHostFree(pin_in[k]);
        if (pin_out[k]) (void)hipHostFree(pin_out[k]);
        st[k] = nullptr; done[k] = nullptr; dev[k] = nullptr; pin_in[k] = nullptr; pin_out[k] = nullptr;
    }
    bytes = 0;
}
}  // namespace agx

namespace {

// one cached set per device, handed to one call at a time; a second concurrent call gets nullptr and builds its own
std::mutex g_stage_mu[kMaxDevices];
staging_set g_stage_pool[kMaxDevices];

staging_set* acquire_staging(int device) {
    if (device < 0 || device >= kMaxDevices) return nullptr;
    return g_stage_mu[device].try_lock() ? &g_stage_pool[device] : nullptr;
}
void release_staging(int device) { g_stage_mu[device].unlock(); }
// frees the pooled set of `device` unless a call holds it (agx_ntt_release_caches)
void release_idle_staging(int device) {
    if (!g_stage_mu[device].try_lock()) return;
    int cur = -1;
    if (g_stage_pool[device].bytes && hipGetDevice(&cur) == hipSuccess && hipSetDevice(device) == hipSuccess) {
        g_stage_pool[device].destroy();
        (void)hipSetDevice(cur);
    }
    g_stage_mu[device].unlock();
}

unsigned stage_workers() {
    const unsigned hc = std::thread::hardware_concurrency();
    unsigned cap = 4;
    if (const char* v = std::getenv("AGX_STAGE_WORKERS")) cap = (unsigned)std::max(1, std::atoi(v));   // tuning knob (tools/host_stream_bench.py)
    return std::max(1u, std::min(cap, hc / 2));
}

template <class F>
void parallel_for(uint64_t items, unsigned workers, F&& fn) {
    if (workers <= 1 || items < 2) { fn(0, items); return; }
    const unsigned t = (unsigned)std::min<uint64_t>(workers, items);
    std::vector<std::thread> pool;
    pool.reserve(t - 1);
    for (unsigned w = 1; w < t; ++w) pool.emplace_back([&, w] { fn(items * w / t, items * (w + 1) / t); });
    fn(0, items / t);
    for (std::thread& th : pool) th.join();
}

void parallel_memcpy(void* dst, const void* src, size_t bytes, unsigned workers) {
    const uint64_t blocks = (bytes + 4095) / 4096;      // split on page multiples
    parallel_for(blocks, workers, [&](uint64_t lo, uint64_t hi) {
        const size_t b0 = (size_t)lo * 4096, b1 = std::min<size_t>(bytes, (size_t)hi * 4096);
        if (b1 > b0) std::memcpy(static_cast<char*>(dst) + b0, static_cast<const char*>(src) + b0, b1 - b0);
    });
}

}  // namespace

namespace agx {

int host_stream_pipeline(const agx_ntt_plan* plan, const uint64_t* in, const uint64_t* in2, uint64_t* out, uint64_t num_frames,
                         bool inverse, staging_set* own) {
    if (!plan || !in || !in2 || !out) return AGX_ERR_NULL_POINTER;
    if (plan->num_primes != 1) return AGX_ERR_BAD_ARGUMENT;   // one modulus per stream, as the reference (ntt.cpp:143-144)
    if (inverse && !plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (int rc = check_plan(plan)) return rc;   // staging memory is allocated on the current device
    if (num_frames == 0) return AGX_OK;
    auto transform = [&](uint64_t* d, uint64_t frames, hipStream_t s) {
        return inverse ? agx_ntt_inverse(plan, d, d, frames, s) : agx_ntt_forward(plan, d, d, frames, s);
    };
    const size_t n = plan->n, row = n * sizeof(uint64_t), half = row / 2;
    if (num_frames * row <= ((size_t)4 << 20)) {
        // small inputs: staging buffers and streams would cost more than they hide
        uint64_t* d = nullptr;
        hipError_t se = hipMalloc(reinterpret_cast<void**>(&d), row * num_frames);
        int src = AGX_OK;
        if (se == hipSuccess) se = hipMemcpy2D(d, row, in, row, half, num_frames, hipMemcpyHostToDevice);
        if (se == hipSuccess) se = hipMemcpy2D(reinterpret_cast<char*>(d) + half, row, reinterpret_cast<const char*>(in2) + half, row, half, num_frames, hipMemcpyHostToDevice);
        if (se == hipSuccess) {
            src = transform(d, num_frames, nullptr);
            if (src == AGX_OK) se = hipMemcpy(out, d, row * num_frames, hipMemcpyDeviceToHost);
        }
        if (d) (void)hipFree(d);
        if (src != AGX_OK) return src;
        return se == hipSuccess ? AGX_OK : hip_fail(se);
    }
    // Pipeline: 3 slots of {pinned in, pinned out, device} on 3 streams.  The ABI takes pageable host pointers, so every
    // byte is also copied once into and once out of pinned memory by the CPU; at ~12 GiB/s per core that staging, not
    // PCIe, is the bottleneck of a single-threaded pipeline (tools/host_stream_bench.py).  Hence: the staging copies of a
    // chunk are split over a few worker threads, the drain of chunk c-3 runs beside the staging of chunk c, and the
    // pinned / device slots and streams are kept between calls (allocating 192 MiB of pinned memory costs more than moving
    // 1 GiB through it): in the caller's own set (a group's shard), else in a per-device pool.
    // Whatever leaves this function -- a status, an exception from std::thread -- `lease` first waits for the slot streams and
    // then gives the pooled set back / frees the temporary one (a throw used to leave the pool's lock held for good).
    struct lease_t {
        staging_set* set = nullptr;
        staging_set local;
        int pooled_device = -1;
        ~lease_t() {
            if (set)
                for (int k = 0; k < staging_set::kSlots; ++k)
                    if (set->st[k]) (void)hipStreamSynchronize(set->st[k]);
            if (pooled_device >= 0) release_staging(pooled_device);
            local.destroy();
        }
    } lease;
    if (own) {
        lease.set = own;
    } else if (staging_set* pooled = acquire_staging(plan->device)) {
        lease.set = pooled;
        lease.pooled_device = plan->device;
    } else {
        lease.set = &lease.local;
    }
    staging_set* set = lease.set;
    hipError_t e = set->ensure(kStageChunkBytes);
    int rc = AGX_OK;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(num_frames, kStageChunkBytes / row));
    const uint64_t nchunks = (num_frames + chunk - 1) / chunk;
    const int slots = (int)std::min<uint64_t>(staging_set::kSlots, nchunks);
    const unsigned workers = stage_workers();
    auto frames_of = [&](uint64_t c) { return std::min<uint64_t>(chunk, num_frames - c * chunk); };
    auto copy_out = [&](uint64_t c) {   // chunk c's results: pinned -> caller's buffer (ntt.cpp:628-633)
        parallel_memcpy(out + c * chunk * n, set->pin_out[c % slots], frames_of(c) * row, workers);
    };
    auto drain = [&](uint64_t c) {
        hipError_t de = hipEventSynchronize(set->done[c % slots]);
        if (de == hipSuccess) copy_out(c);
        return de;
    };
    for (uint64_t c = 0; c < nchunks && e == hipSuccess && rc == AGX_OK; ++c) {
        const int k = (int)(c % slots);
        joining_thread drainer;      // joined on every path out of this iteration
        if (c >= (uint64_t)slots) {
            // slot k still belongs to chunk c-slots: done[k] (recorded behind its download) says its upload source
            // pin_in[k] is free again and its results sit in pin_out[k]
            e = hipEventSynchronize(set->done[k]);
            if (e != hipSuccess) break;
            drainer = joining_thread([&, c] { copy_out(c - slots); });     // beside the staging of chunk c
        }
        const uint64_t f = frames_of(c);
        const uint64_t* a = in + c * chunk * n;
        const uint64_t* b = in2 + c * chunk * n;
        if (a == b) {
            parallel_memcpy(set->pin_in[k], a, f * row, workers);
        } else {
            // lower half of each frame from `in`, upper half from `in2` (src/kernel/ntt.cpp:584-590)
            parallel_for(f, workers, [&](uint64_t lo, uint64_t hi) {
                for (uint64_t i = lo; i < hi; ++i) {
                    std::memcpy(reinterpret_cast<char*>(set->pin_in[k]) + i * row, reinterpret_cast<const char*>(a) + i * row, half);
                    std::memcpy(reinterpret_cast<char*>(set->pin_in[k]) + i * row + half, reinterpret_cast<const char*>(b) + i * row + half, half);
                }
            });
        }
        e = hipMemcpyAsync(set->dev[k], set->pin_in[k], f * row, hipMemcpyHostToDevice, set->st[k]);
        if (e == hipSuccess) rc = transform(set->dev[k], f, set->st[k]);
        drainer.join();      // pin_out[k] must be empty before this chunk's download may land in it
        if (e == hipSuccess && rc == AGX_OK) e = hipMemcpyAsync(set->pin_out[k], set->dev[k], f * row, hipMemcpyDeviceToHost, set->st[k]);
        if (e == hipSuccess && rc == AGX_OK) e = hipEventRecord(set->done[k], set->st[k]);
    }
    for (uint64_t c = nchunks > (uint64_t)slots ? nchunks - slots : 0; c < nchunks && e == hipSuccess && rc == AGX_OK; ++c) e = drain(c);
    if (rc != AGX_OK) return rc;
    return e == hipSuccess ? AGX_OK : hip_fail(e);
}

}  // namespace agx

extern "C" {

// Host-resident frames through a device plan with transfers and compute overlapped: the GPU
// analogue of the reference's streaming ntt_input_kernel / ntt_output_kernel pair
// (src/kernel/ntt.cpp:508-640).  Three slots of pinned staging + device memory rotate over three
// streams: while slot k computes, slot k+1 uploads and the host thread assembles slot k+2
// (lower half of each frame from `in`, upper half from `in2`, src/kernel/ntt.cpp:584-590).
int agx_ntt_forward_host_stream(const agx_ntt_plan* plan, const uint64_t* in, const uint64_t* in2, uint64_t* out,
                                uint64_t num_frames) {
    return guarded([&] { return host_stream_pipeline(plan, in, in2, out, num_frames, false, nullptr); });      // std::thread / std::vector inside may throw
}

// the inverse transform through the same pipeline (bit-reversed order in, natural order out; no operand pairing: the reference has no
// inverse path)
int agx_ntt_inverse_host_stream(const agx_ntt_plan* plan, const uint64_t* in, uint64_t* out, uint64_t num_frames) {
    return guarded([&] { return host_stream_pipeline(plan, in, in, out, num_frames, true, nullptr); });
}

// One-shot calls usually repeat with the same (n, modulus, tables): building a plan verifies every table
// entry (a 128-bit divide each) and uploads four tables, which costs tens of milliseconds, so the last
// plan of each device is kept and reused while the caller's tables still compare equal word for word.
// One slot and one lock PER DEVICE: calls on different GPUs neither evict each other's plan nor serialise.
namespace {
// what a cached one-shot plan or group was built from: the caller's tables are compared word for word
struct oneshot_key {
    uint32_t n = 0;
    uint64_t q = 0;
    std::vector<uint64_t> tw, pre;
    bool matches(uint32_t n_, uint64_t q_, const uint64_t* tw_, const uint64_t* pre_) const {
        return n == n_ && q == q_ && std::memcmp(tw.data(), tw_, (size_t)n_ * 8) == 0 && std::memcmp(pre.data(), pre_, (size_t)n_ * 8) == 0;
    }
    void assign(uint32_t n_, uint64_t q_, const uint64_t* tw_, const uint64_t* pre_) { *this = oneshot_key{n_, q_, {tw_, tw_ + n_}, {pre_, pre_ + n_}}; }
};
struct oneshot_cache {
    std::mutex mu;
    agx_ntt_plan* plan = nullptr;
    oneshot_key key;
};
oneshot_cache g_oneshot[kMaxDevices];

// AGX_NTT_DEVICES=0,1,2,3 in the environment: the one-shot call deals its frames to those devices (a group, include/agx_ntt.h section 5)
// instead of running on the current one -- the reference's NUM_NTT_COMPUTE_UNITS replication (src/kernel/ntt.cpp:8-12, 526-536) for a
// caller that cannot change its code.  One cached group, rebuilt when (n, modulus, tables, device list) change.
struct oneshot_group_cache {
    std::mutex mu;
    agx_ntt_group* group = nullptr;
    oneshot_key key;
    std::vector<int> devices;
};
oneshot_group_cache g_oneshot_group;

void env_device_list(std::vector<int>& out) {
    out.clear();
    const char* v = std::getenv("AGX_NTT_DEVICES");
    if (!v || !*v) return;
    for (const char* p = v; *p;) {
        char* end = nullptr;
        const long d = std::strtol(p, &end, 10);
        if (end == p) {      // not a number: a device id the group will refuse
            out.assign(1, -1);
            return;
        }
        out.push_back((int)d);
        p = end;
        while (*p == ',' || *p == ' ') ++p;
    }
}
}  // namespace

int agx_ntt_forward_host(const uint64_t* in, const uint64_t* in2, const uint64_t* modulus,
                         const uint64_t* twiddles, const uint64_t* precons, uint64_t* out,
                         uint32_t n, uint32_t num_frames) {
    if (!in || !in2 || !out) return AGX_ERR_NULL_POINTER;
    int rc = check_create_args(n, 1, modulus, twiddles, precons, nullptr, nullptr);      // the rules of the plan this call builds
    if (rc) return rc;
    if (num_frames == 0) return AGX_OK;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return AGX_ERR_NO_DEVICE;
    return guarded([&]() -> int {
        std::vector<int> devices;
        env_device_list(devices);
        if (!devices.empty()) {
            oneshot_group_cache& c = g_oneshot_group;
            std::lock_guard<std::mutex> lock(c.mu);
            if (!(c.group && c.devices == devices && c.key.matches(n, modulus[0], twiddles, precons))) {
                agx_ntt_group* g = nullptr;
                if ((rc = agx_ntt_group_create(&g, devices.data(), (uint32_t)devices.size(), n, 1, modulus, twiddles, precons, nullptr, nullptr))) return rc;
                agx_ntt_group_destroy(c.group);
                c.group = g;
                c.key.assign(n, modulus[0], twiddles, precons);
                c.devices = devices;
            }
            return agx_ntt_group_forward_host(c.group, in, in2, out, num_frames);
        }
        if (dev < 0 || dev >= kMaxDevices) {      // no cache slot: build, use, destroy
            agx_ntt_plan* plan = nullptr;
            if ((rc = build_plan(&plan, n, 1, modulus, nullptr, twiddles, precons, nullptr, nullptr))) return rc;
            rc = agx_ntt_forward_host_stream(plan, in, in2, out, num_frames);
            free_plan(plan);
            return rc;
        }
        oneshot_cache& c = g_oneshot[dev];
        std::lock_guard<std::mutex> lock(c.mu);    // one-shot calls are synchronous; those of one device also serialise
        if (!(c.plan && c.key.matches(n, modulus[0], twiddles, precons))) {
            agx_ntt_plan* plan = nullptr;
            if ((rc = build_plan(&plan, n, 1, modulus, nullptr, twiddles, precons, nullptr, nullptr))) return rc;
            free_plan(c.plan);
            c.plan = plan;
            c.key.assign(n, modulus[0], twiddles, precons);
        }
        return agx_ntt_forward_host_stream(c.plan, in, in2, out, num_frames);
    });
}

// Frees what the library keeps between calls: the one-shot plans and the pinned / device staging buffers of every device
// (192 MiB pinned + 96 MiB device memory per device that has streamed host frames).  Call it before hipDeviceReset or at
// shutdown; calls running at the same time keep what they hold (a busy staging set is skipped).  Later calls rebuild on demand.
int agx_ntt_release_caches(void) {
    {
        std::lock_guard<std::mutex> lock(g_oneshot_group.mu);
        agx_ntt_group_destroy(g_oneshot_group.group);      // joins its workers; each frees its shard on its own device
        g_oneshot_group.group = nullptr;
        g_oneshot_group.key = oneshot_key{};
    }
    for (int d = 0; d < kMaxDevices; ++d) {
        {
            std::lock_guard<std::mutex> lock(g_oneshot[d].mu);
            free_plan(g_oneshot[d].plan);
            g_oneshot[d].plan = nullptr;
            g_oneshot[d].key = oneshot_key{};
        }
        release_idle_staging(d);
    }
    return AGX_OK;
}

// ---- number theory for callers that build their own tables: no device involved ----

int agx_ntt_find_primes(uint32_t bits, uint32_t n, uint32_t count, uint64_t* primes_out) {
    if (!primes_out) return AGX_ERR_NULL_POINTER;
    if (int rc = check_size(n)) return rc;
    if (bits < 2 || bits > 62) return AGX_ERR_BAD_ARGUMENT;
    return guarded([&]() -> int {
        std::vector<uint64_t> v = find_ntt_primes(bits, n, count);
        if (v.size() < count) return AGX_ERR_BAD_ARGUMENT;
        std::memcpy(primes_out, v.data(), sizeof(uint64_t) * count);
        return AGX_OK;
    });
}

int agx_ntt_min_root(uint64_t q, uint32_t n, uint64_t* psi_out) {
    if (!psi_out) return AGX_ERR_NULL_POINTER;
    if (int rc = check_size(n)) return rc;
    if (int rc = check_modulus(q, n)) return rc;
    if (!is_prime_u64(q)) return AGX_ERR_BAD_MODULUS;
    const uint64_t r = min_primitive_root_2n(q, n);
    if (!r) return AGX_ERR_BAD_ROOT;
    *psi_out = r;
    return AGX_OK;
}

int agx_ntt_galois_element(uint32_t n, int64_t step, uint32_t* galois_elt) {
    if (!galois_elt) return AGX_ERR_NULL_POINTER;
    if (int rc = check_size(n)) return rc;
    const uint32_t mask = 2u * n - 1u;
    uint32_t base = 5u;
    if (step < 0) {      // 5^-1 mod 2n: Newton's iteration on the odd 5 doubles the correct low bits (3 -> 6 -> 12 -> 24 >= 16)
        for (int it = 0; it < 3; ++it) base *= 2u - 5u * base;
    }
    base &= mask;
    uint32_t g = 1u;
    for (uint64_t e = step < 0 ? 0 - (uint64_t)step : (uint64_t)step; e; e >>= 1, base = (base * base) & mask)      // factors below 2^16
        if (e & 1u) g = (g * base) & mask;
    *galois_elt = g;
    return AGX_OK;
}

static int make_tables_common(uint64_t q, uint64_t psi, uint32_t n, uint64_t* tw, uint64_t* pre, bool inverse) {
    if (!tw || !pre) return AGX_ERR_NULL_POINTER;
    if (int rc = check_size(n)) return rc;
    if (int rc = check_modulus(q, n)) return rc;
    if (!is_prime_u64(q)) return AGX_ERR_BAD_MODULUS;
    if (!is_primitive_root_2n(psi, q, n)) return AGX_ERR_BAD_ROOT;
    power_tables_bitrev(q, inverse ? inv_mod(psi, q) : psi, n, tw, pre);
    return AGX_OK;
}

int agx_ntt_make_tables(uint64_t q, uint64_t psi, uint32_t n, uint64_t* twiddles, uint64_t* precons) {
    return make_tables_common(q, psi, n, twiddles, precons, false);
}

int agx_ntt_make_inverse_tables(uint64_t q, uint64_t psi, uint32_t n, uint64_t* inv_twiddles, uint64_t* inv_precons) {
    return make_tables_common(q, psi, n, inv_twiddles, inv_precons, true);
}

}  // extern "C"
