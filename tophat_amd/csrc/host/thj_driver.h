// thj_driver.h -- what the two shard drivers (segment_juncs, long_spanning_reads) share around the device: the contexts and their
// start-up, the GPU's lock with its accounting, read packing, a shard's id range as the C ABI takes it.
#pragma once
#include "thj_hostio.h"

namespace thjh {

// one GPU context: created on a side thread while the first shards are parsed, and the lock that serialises the device calls of
// the host workers feeding it
struct Gpu {
    int device = 0;
    thj_ctx* ctx = nullptr;
    std::future<thj_ctx*> fut;
    std::mutex mu;
};

// Every visible GPU (THJ_GPUS caps the count, THJ_DEVICE picks a single device), each context created -- and warmed with `warm`
// (THJ_WARM_* bits, 0: not at all) -- on its own thread.
// THJ_CTX_PER_GPU=k: k contexts (streams, arenas, tables) on every device, each a rank of its own -- a shard's host-to-device
// copies and stream round trips then overlap another shard's kernels on the same GPU.  One per device on several devices: a
// communicator is either all-RCCL or all-loopback.
inline std::vector<std::unique_ptr<Gpu>> start_contexts(int default_per_gpu, int warm, const PhaseTimer& timer) {
    int n_dev = 1, first = 0;
    if (getenv("THJ_DEVICE")) first = atoi(getenv("THJ_DEVICE"));
    else {
        n_dev = thj_device_count();
        if (n_dev < 1) die("Error: %s\n", thj_last_error());
        if (getenv("THJ_GPUS") && atoi(getenv("THJ_GPUS")) >= 1) n_dev = std::min(n_dev, atoi(getenv("THJ_GPUS")));
    }
    int per = getenv("THJ_CTX_PER_GPU") ? atoi(getenv("THJ_CTX_PER_GPU")) : default_per_gpu;
    if (n_dev > 1) per = 1;
    per = std::max(1, std::min(8, per));
    std::vector<std::unique_ptr<Gpu>> gpus;
    for (int d = 0; d < n_dev * per; ++d) {
        gpus.emplace_back(new Gpu());
        Gpu& g = *gpus.back();
        g.device = first + d / per;
        g.fut = std::async(std::launch::async, [dev = g.device, warm, wall0 = timer.wall0]() {
            thj_ctx* c = nullptr;
            if (thj_ctx_create(dev, nullptr, &c)) die("Error: %s\n", thj_last_error());
            if (warm && thj_ctx_warm(c, warm)) die("Error: %s\n", thj_last_error());
            if (getenv("THJ_TIMING")) fprintf(stderr, "[timing] a device context ready after       %8.3f s of the process\n", std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count() - wall0);
            return c;
        });
    }
    return gpus;
}

// Holds a GPU's lock: the wait for it goes to work clock 1, the time it is held -- the device calls -- to work clock 2.
struct GpuLock {
    WorkClock& work;
    const long long t_wait = WorkClock::now();
    std::lock_guard<std::mutex> lk;
    long long t_held;
    GpuLock(Gpu& g, WorkClock& w) : work(w), lk(g.mu) { work.add(1, t_wait); t_held = WorkClock::now(); }
    ~GpuLock() { work.add(2, t_held); }
};

// Reads as the kernels take them: three bit planes of W 64-base words per read (thj_reads_pack), lengths and -- where asked for --
// quality rows of `stride` bytes.  read_off[r] .. read_off[r + 1] = read r's share of `bases` (and of `quals`).
struct PackedReads {
    int W = 1, stride = 0;
    std::vector<uint64_t> planes; std::vector<uint16_t> lens; std::vector<uint8_t> quals;
};
inline PackedReads pack_reads(const std::vector<int64_t>& read_off, const std::string& bases, size_t max_len, const std::string* quals = nullptr) {
    PackedReads p;
    const int64_t n = (int64_t)read_off.size() - 1;
    p.W = std::max(1, (int)((max_len + 63) / 64));
    p.planes.resize((size_t)n * 3 * p.W);
    p.lens.resize((size_t)n);
    if (thj_reads_pack(n, read_off.data(), bases.data(), p.W, p.planes.data(), p.lens.data())) die("Error: %s\n", thj_last_error());
    if (!quals) return p;
    p.stride = (int)((max_len + 3) / 4 * 4);
    p.quals.assign((size_t)n * p.stride, 0);
    for (int64_t r = 0; r < n; ++r) memcpy(p.quals.data() + (size_t)r * p.stride, quals->data() + read_off[(size_t)r], (size_t)(read_off[(size_t)r + 1] - read_off[(size_t)r]));
    return p;
}

// a shard's id bound as the 32-bit argument of the ingest calls
inline uint32_t clamp_id32(uint64_t id) { return id > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)id; }

}  // namespace thjh
