// thj_bamout.hip -- the device side of long_spanning_reads' BAM writer (print_bamhit, bwt_map.cpp:1888-2093; bam_write1 ->
// bgzf_write -> deflate_block, samtools-0.1.18 bam.c:207-236, bgzf.c:287-349):
//   thj_k_bam_shapes / thj_k_bam_write   the pass's alignments as BAM records, from the device records and the reads' own BAM
//                                        records (both already in HBM), back to back in output order;
//   thj_k_bam_write_fusion               the fusion alignments among them (two records with XF:Z each, thj_bamenc_fusion.h): a wave
//                                        per alignment over the list thj_k_bam_shapes<true> made, which thj_k_bam_write<true> skips;
//   thj_k_deflate                        one workgroup of 16 waves per BGZF member: DEFLATE stream + CRC-32 (thj_deflate_core.h);
//   thj_k_pack_members                   the members' compressed bytes back to back for one copy down.
// The host plans where members end (bam_write1's bgzf_flush_try rule needs only record sizes), adds the 18 + 8 bytes of BGZF
// envelope and writes; it never sees the uncompressed records.  HBM-bound byte work; no MFMA.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/thj.h"
#include "thj_ctx.h"
#include "thj_scan.h"

#define THJ_DFN __device__ __forceinline__
#include "thj_deflate_core.h"
#include "thj_bamenc_core.h"
#include "thj_bamenc_fusion.h"

namespace {

struct GpuX {
    int tid, lane, wave;
    __device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
    __device__ __forceinline__ uint32_t shfl(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src); }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(src)); }
    __device__ __forceinline__ uint32_t incl_scan(uint32_t v) {
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
        return v;
    }
    __device__ __forceinline__ uint32_t wave_max(uint32_t v) {
        for (int o = 32; o; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o); v = w > v ? w : v; }
        return v;
    }
    __device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
        for (int o = 32; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
        return v;
    }
    // lanes of a wave run in lockstep and the LDS serves a wave's requests in order: only the compiler has to be kept from moving
    // memory operations across the point
    __device__ __forceinline__ void wsync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ uint32_t lds_add(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
    __device__ __forceinline__ void lds_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
    __device__ __forceinline__ void glb_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
    __device__ __forceinline__ unsigned long long clock() { return wall_clock64(); }
};

// member m of the launch = stream[ends[first + m - 1] .. ends[first + m]) (0 before the first)
__global__ __launch_bounds__(dfl::NT) void thj_k_deflate(const uint8_t* __restrict__ stream, const int64_t* __restrict__ ends, int first, uint32_t* __restrict__ tokens,
                                                         uint32_t* __restrict__ out, uint32_t* __restrict__ results, unsigned long long* __restrict__ tm) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[dfl::L_END];
    const int m = (int)blockIdx.x;
    const int64_t b = first + m ? ends[first + m - 1] : 0, e = ends[first + m];
    GpuX x{(int)threadIdx.x, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6)};
    dfl::deflate_member(x, lds, stream + b, (uint32_t)(e - b), tokens + ((size_t)m << 16), out + ((size_t)m << 14), results + 4 * (size_t)m, tm ? tm + 16 * (size_t)m : nullptr);
}

// results[4m + 3] = where member m's bytes start in the packed buffer (one workgroup; n <= 4096)
__global__ __launch_bounds__(1024) void thj_k_member_offsets(uint32_t* __restrict__ results, int n) {
    __shared__ uint32_t part[1024];
    const int t = (int)threadIdx.x;
    uint32_t v[4], s = 0;
    for (int k = 0; k < 4; ++k) { const int m = 4 * t + k; v[k] = m < n ? results[4 * m] : 0u; s += v[k]; }
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) { const uint32_t a = t >= o ? part[t - o] : 0u; __syncthreads(); part[t] += a; __syncthreads(); }
    uint32_t at = part[t] - s;
    for (int k = 0; k < 4; ++k) { const int m = 4 * t + k; if (m < n) results[4 * m + 3] = at; at += v[k]; }
}
__global__ __launch_bounds__(256) void thj_k_pack_members(const uint8_t* __restrict__ out, const uint32_t* __restrict__ results, uint8_t* __restrict__ packed) {
    const int m = (int)blockIdx.x;
    const uint32_t n = results[4 * m], at = results[4 * m + 3];
    const uint8_t* src = out + ((size_t)m << 16);
    uint8_t* dst = packed + at;
    // word copies where the destination allows
    const uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3u)) & 3u) < n ? (uint32_t)((4 - ((uintptr_t)dst & 3u)) & 3u) : n;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t words = (n - head) >> 2;
    for (uint32_t w = threadIdx.x; w < words; w += 256) { uint32_t v; memcpy(&v, src + head + 4 * w, 4); *(uint32_t*)(dst + head + 4 * w) = v; }
    const uint32_t done = head + 4 * words;
    if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

// FUSION = false: every alignment is one record; flag bit 0 = one needs the host encoder, bit 2 = because it is a fusion alignment.
// FUSION = true (a pass that holds fusion alignments, contig names on the context): size[i] = both records' bytes, size2[i] = the second
// record's (0: a plain alignment); the fusion alignments' indices go to list, one reservation per wave.
template <bool FUSION>
__global__ __launch_bounds__(256) void thj_k_bam_shapes(const thj_aln* __restrict__ alns, int64_t n, const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc, int32_t n_rows,
                                                        size_t infl_bytes, int32_t n_ref, uint32_t* __restrict__ size, long long* __restrict__ rid, unsigned int* __restrict__ flag,
                                                        const uint32_t* __restrict__ name_off, uint32_t* __restrict__ size2, uint32_t* __restrict__ list, unsigned int* __restrict__ n_list) {
    if constexpr (!FUSION) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            const thj_aln& a = alns[i];
            if (a.read_idx >= (uint32_t)n_rows || a.ref_id < 1 || a.ref_id > (uint32_t)n_ref || (size_t)loc[a.read_idx] + 36 > infl_bytes) { atomicOr(flag, 2u); size[i] = 0; rid[i] = 0; continue; }
            const bamenc::Shape s = bamenc::record_shape(a, infl + loc[a.read_idx] + 4);
            if (s.host_only) atomicOr(flag, s.fusion ? 4u : 1u);
            size[i] = s.size; rid[i] = s.rid;
        }
    } else {
        // whole waves go round: the ballot needs every lane of a wave that has work
        const uint32_t lane = threadIdx.x & 63u;
        for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = i0 + lane;
            bool listed = false;
            if (i < n) {
                const thj_aln& a = alns[i];
                if (a.read_idx >= (uint32_t)n_rows || a.ref_id < 1 || a.ref_id > (uint32_t)n_ref || (size_t)loc[a.read_idx] + 36 > infl_bytes) {
                    atomicOr(flag, 2u); size[i] = 0; size2[i] = 0; rid[i] = 0;
                } else {
                    const bamenc::FusionShape f = bamenc::fusion_shape(a, infl + loc[a.read_idx] + 4, name_off, n_ref);
                    if (f.host_only) atomicOr(flag, 1u);
                    size[i] = f.size1 + f.size2; size2[i] = f.size2; rid[i] = f.rid;
                    listed = !f.host_only && f.size2 != 0;
                }
            }
            const uint64_t m = __ballot(listed);
            if (m) {
                const int first = __builtin_ctzll(m);
                unsigned int base = 0;
                if ((int)lane == first) base = atomicAdd(n_list, (unsigned int)__builtin_popcountll(m));
                base = (unsigned int)__shfl((int)base, first);
                if (listed) list[base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
            }
        }
    }
}
// FUSION: the alignments thj_k_bam_write_fusion takes (size2 != 0) are passed over
template <bool FUSION>
__global__ __launch_bounds__(256) void thj_k_bam_write(const thj_aln* __restrict__ alns, int64_t n, const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc,
                                                       const int32_t* __restrict__ tid_of_ref, const unsigned long long* __restrict__ off, uint8_t* __restrict__ out,
                                                       const uint32_t* __restrict__ size2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (FUSION && size2[i] != 0) continue;
        const thj_aln& a = alns[i];
        const uint8_t* raw = infl + loc[a.read_idx] + 4;
        const bamenc::Shape s = bamenc::record_shape(a, raw);
        bamenc::record_write(a, raw, s, tid_of_ref[a.ref_id - 1], out + off[i]);
    }
}
// a wave per listed alignment: both records back to back at the alignment's offset.  No __restrict__ here: with it the compiler hoists
// whatever the two records share out of fusion_write's loop and runs out of scalar registers (67 SGPR spills; none without)
__global__ __launch_bounds__(256) void thj_k_bam_write_fusion(const thj_aln* alns, const uint32_t* list, uint32_t n_list, const uint8_t* infl, const uint32_t* loc,
                                                              const int32_t* tid_of_ref, const uint8_t* names, const uint32_t* name_off, const unsigned long long* off, uint8_t* out) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= n_list) return;
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[w]);
    GpuX x{(int)threadIdx.x, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6)};
    const thj_aln& a = alns[i];
    bamenc::fusion_write(x, a, infl + loc[a.read_idx] + 4, names, name_off, tid_of_ref, out + off[i]);
}


int ensure_bam(thj_ctx* c, size_t bytes) {
    if (bytes <= c->bam_cap) return THJ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->d_bam) (void)hipFree(c->d_bam);
    c->d_bam = nullptr; c->bam_cap = 0;
    const size_t cap = bytes + bytes / 4 + 4096;
    HIPCHK(hipMalloc((void**)&c->d_bam, cap));
    c->bam_cap = cap;
    return THJ_OK;
}
int ensure_tmp(thj_ctx* c, size_t bytes) {
    if (bytes <= c->bam_tmp_cap) return THJ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->d_bam_tmp) (void)hipFree(c->d_bam_tmp);
    c->d_bam_tmp = nullptr; c->bam_tmp_cap = 0;
    HIPCHK(hipMalloc(&c->d_bam_tmp, bytes));
    c->bam_tmp_cap = bytes;
    return THJ_OK;
}

}  // namespace

// the stream grows and keeps what it holds (the accepted-hits pass appends piece after piece)
int thj_bam_stream_reserve(thj_ctx* c, size_t bytes) {
    if (bytes <= c->bam_cap) return THJ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t cap = bytes + bytes / 2 + 4096;
    uint8_t* n = nullptr;
    HIPCHK(hipMalloc((void**)&n, cap));
    if (c->d_bam && c->bam_bytes > 0) HIPCHK(hipMemcpy(n, c->d_bam, (size_t)c->bam_bytes, hipMemcpyDeviceToDevice));
    if (c->d_bam) (void)hipFree(c->d_bam);
    c->d_bam = n; c->bam_cap = cap;
    return THJ_OK;
}

void thj_bamout_free(thj_ctx* c) {
    if (c->d_bam) (void)hipFree(c->d_bam);
    if (c->d_bam_tmp) (void)hipFree(c->d_bam_tmp);
    if (c->d_contig_names) (void)hipFree(c->d_contig_names);
    if (c->d_contig_name_off) (void)hipFree(c->d_contig_name_off);
    if (c->d_contig_name_sorted) (void)hipFree(c->d_contig_name_sorted);
    c->d_bam = nullptr; c->d_bam_tmp = nullptr; c->bam_cap = c->bam_tmp_cap = 0; c->bam_bytes = 0;
    c->d_contig_names = nullptr; c->d_contig_name_off = nullptr; c->d_contig_name_sorted = nullptr; c->n_contig_names = 0;
}

namespace {
// thj_span_bam_encode (fusion == false: one record per alignment, n entries) and thj_span_bam_encode_records
int bam_encode(thj_ctx* c, const char* who, const thj_span_batch* batch, const int32_t* tid_of_ref, int32_t n_ref, bool fusion, int64_t rec_cap, uint32_t* rec_size,
               int64_t* rec_id, int64_t* n_records, int64_t* total_bytes) {
    const OwnedSpanBatch* ob = (const OwnedSpanBatch*)batch;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->bam_bytes = 0; *total_bytes = 0;
    if (n_records) *n_records = 0;
    const int64_t n = c->n_alns;
    if (n == 0) return THJ_OK;
    if (rec_cap < n) { thj_set_error("%s: room for %lld records, the pass has %lld alignments", who, (long long)rec_cap, (long long)n); return THJ_EINVAL; }
    if (!ob->ptrs[6] || !ob->ptrs[7]) { thj_set_error("%s: the batch holds no read records (thj_ingest_span_batch makes the batches this takes)", who); return THJ_EFALLBACK; }
    void* d_alns = nullptr;
    int rc = thj_span_compact_device(c, &d_alns);
    if (rc == THJ_EFALLBACK) { thj_set_error("%s: the pass's records could not be compacted on the device", who); return THJ_EFALLBACK; }
    if (rc) return rc;
    void *d_size = nullptr, *d_rid = nullptr, *d_off = nullptr, *d_tid = nullptr, *d_tmp = nullptr, *d_size2 = nullptr, *d_list = nullptr;
    auto done = [&](int code) {
        (void)hipStreamSynchronize(c->stream);
        thj_dev_release(c, d_alns); thj_dev_release(c, d_size); thj_dev_release(c, d_rid); thj_dev_release(c, d_off); thj_dev_release(c, d_tid); thj_dev_release(c, d_tmp);
        thj_dev_release(c, d_size2); thj_dev_release(c, d_list);
        return code;
    };
#define BAM_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { thj_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); return done(THJ_EHIP); } } while (0)
    const size_t tmp_bytes = thj_scan::scratch_bytes(n, 8);            // (thj_scan.h: not hipcub::DeviceScan)
    if (thj_dev_alloc(c, &d_size, (size_t)n * 4 + 16) || thj_dev_alloc(c, &d_rid, (size_t)n * 8) || thj_dev_alloc(c, &d_off, (size_t)n * 8) ||
        thj_dev_alloc(c, &d_tid, (size_t)n_ref * 4) || thj_dev_alloc(c, &d_tmp, tmp_bytes + 16)) return done(THJ_EHIP);
    unsigned int* d_flag = (unsigned int*)((char*)d_size + (size_t)n * 4);
    BAM_HIP(hipMemsetAsync(d_flag, 0, 4, c->stream));
    BAM_HIP(hipMemcpyAsync(d_tid, tid_of_ref, (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream));
    int64_t grid = (n + 255) / 256; if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(thj_k_bam_shapes<false>, dim3((unsigned)grid), dim3(256), 0, c->stream, (const thj_aln*)d_alns, n, (const uint8_t*)ob->ptrs[6], (const uint32_t*)ob->ptrs[7],
                       batch->n_reads, ob->reads_infl_bytes, n_ref, (uint32_t*)d_size, (long long*)d_rid, d_flag, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                       (unsigned int*)nullptr);
    BAM_HIP(hipGetLastError());
    thj_scan::exclusive_sum<uint32_t, unsigned long long>(c->stream, (const uint32_t*)d_size, (unsigned long long*)d_off, n, d_tmp);
    unsigned int flag = 0; unsigned long long last_off = 0;
    BAM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    BAM_HIP(hipMemcpyAsync(&last_off, (unsigned long long*)d_off + (n - 1), 8, hipMemcpyDeviceToHost, c->stream));
    BAM_HIP(hipMemcpyAsync(rec_size, d_size, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    BAM_HIP(hipMemcpyAsync(rec_id, d_rid, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    BAM_HIP(hipStreamSynchronize(c->stream));
    if (flag & 2u) { thj_set_error("%s: a record points outside the batch (read index, contig or read record)", who); return done(THJ_EINVAL); }
    if (flag & 1u) {
        thj_set_error("%s: a record of the batch needs the host encoder (%slong MD string, read length)", who, fusion ? "" : "fusion alignment, ");
        return done(THJ_EFALLBACK);
    }
    unsigned int n_list = 0;
    std::vector<uint32_t> h_size2;
    if (flag & 4u) {
        // the pass holds fusion alignments: the shapes again, two records each (thj_bamenc_fusion.h)
        if (!fusion) { thj_set_error("%s: a record of the batch needs the host encoder (fusion alignment)", who); return done(THJ_EFALLBACK); }
        if (!c->d_contig_names || c->n_contig_names != n_ref) {
            thj_set_error("%s: a fusion alignment, and the context holds no names for the run's %d contigs (thj_bam_contig_names_upload)", who, (int)n_ref);
            return done(THJ_EFALLBACK);
        }
        if (n > 0x7FFFFFFFll) { thj_set_error("%s: a fusion alignment in a pass of more than 2^31 alignments", who); return done(THJ_EFALLBACK); }
        if (thj_dev_alloc(c, &d_size2, (size_t)n * 4) || thj_dev_alloc(c, &d_list, (size_t)n * 4 + 16)) return done(THJ_EHIP);
        unsigned int* d_n_list = (unsigned int*)((char*)d_list + (size_t)n * 4);
        BAM_HIP(hipMemsetAsync(d_flag, 0, 4, c->stream));
        BAM_HIP(hipMemsetAsync(d_n_list, 0, 4, c->stream));
        hipLaunchKernelGGL(thj_k_bam_shapes<true>, dim3((unsigned)grid), dim3(256), 0, c->stream, (const thj_aln*)d_alns, n, (const uint8_t*)ob->ptrs[6], (const uint32_t*)ob->ptrs[7],
                           batch->n_reads, ob->reads_infl_bytes, n_ref, (uint32_t*)d_size, (long long*)d_rid, d_flag, (const uint32_t*)c->d_contig_name_off, (uint32_t*)d_size2,
                           (uint32_t*)d_list, d_n_list);
        BAM_HIP(hipGetLastError());
        thj_scan::exclusive_sum<uint32_t, unsigned long long>(c->stream, (const uint32_t*)d_size, (unsigned long long*)d_off, n, d_tmp);
        h_size2.resize((size_t)n);
        BAM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
        BAM_HIP(hipMemcpyAsync(&n_list, d_n_list, 4, hipMemcpyDeviceToHost, c->stream));
        BAM_HIP(hipMemcpyAsync(&last_off, (unsigned long long*)d_off + (n - 1), 8, hipMemcpyDeviceToHost, c->stream));
        BAM_HIP(hipMemcpyAsync(rec_size, d_size, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        BAM_HIP(hipMemcpyAsync(h_size2.data(), d_size2, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        BAM_HIP(hipMemcpyAsync(rec_id, d_rid, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        BAM_HIP(hipStreamSynchronize(c->stream));
        if (flag & 2u) { thj_set_error("%s: a record points outside the batch (read index, contig or read record)", who); return done(THJ_EINVAL); }
        if (flag & 1u) {
            thj_set_error("%s: a record of the batch needs the host encoder (long MD string, read length; a fusion alignment of more than 15 operations, with two fusion points "
                          "or on an unknown second contig)", who);
            return done(THJ_EFALLBACK);
        }
        if ((int64_t)n_list > n || n + (int64_t)n_list > rec_cap) { thj_set_error("%s: room for %lld records, the pass has %lld", who, (long long)rec_cap, (long long)(n + n_list)); return done(THJ_EINVAL); }
    }
    const size_t total = (size_t)last_off + rec_size[n - 1];
    rc = ensure_bam(c, total + 64);
    if (rc) return done(rc);
    if (n_list == 0) {
        hipLaunchKernelGGL(thj_k_bam_write<false>, dim3((unsigned)grid), dim3(256), 0, c->stream, (const thj_aln*)d_alns, n, (const uint8_t*)ob->ptrs[6], (const uint32_t*)ob->ptrs[7],
                           (const int32_t*)d_tid, (const unsigned long long*)d_off, c->d_bam, (const uint32_t*)nullptr);
        BAM_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(thj_k_bam_write<true>, dim3((unsigned)grid), dim3(256), 0, c->stream, (const thj_aln*)d_alns, n, (const uint8_t*)ob->ptrs[6], (const uint32_t*)ob->ptrs[7],
                           (const int32_t*)d_tid, (const unsigned long long*)d_off, c->d_bam, (const uint32_t*)d_size2);
        BAM_HIP(hipGetLastError());
        hipLaunchKernelGGL(thj_k_bam_write_fusion, dim3((n_list + 3u) / 4u), dim3(256), 0, c->stream, (const thj_aln*)d_alns, (const uint32_t*)d_list, (uint32_t)n_list,
                           (const uint8_t*)ob->ptrs[6], (const uint32_t*)ob->ptrs[7], (const int32_t*)d_tid, (const uint8_t*)c->d_contig_names, (const uint32_t*)c->d_contig_name_off,
                           (const unsigned long long*)d_off, c->d_bam);
        BAM_HIP(hipGetLastError());
    }
    BAM_HIP(hipStreamSynchronize(c->stream));
#undef BAM_HIP
    // an entry per record: a fusion alignment's pair of sizes becomes two (from the back, in place)
    if (n_list) {
        int64_t j = n + (int64_t)n_list;
        for (int64_t i = n; i-- > 0;) {
            const uint32_t both = rec_size[i], s2 = h_size2[(size_t)i];
            const int64_t id = rec_id[i];
            if (s2) { --j; rec_size[j] = s2; rec_id[j] = id; }
            --j; rec_size[j] = both - s2; rec_id[j] = id;
        }
    }
    if (n_records) *n_records = n + (int64_t)n_list;
    c->bam_bytes = (int64_t)total; *total_bytes = (int64_t)total;
    return done(THJ_OK);
}
}  // namespace

extern "C" int thj_span_bam_encode(thj_ctx* c, const thj_span_batch* batch, const int32_t* tid_of_ref, int32_t n_ref, uint32_t* rec_size, int64_t* rec_id,
                                   int64_t* total_bytes) {
    if (!c || !batch || !tid_of_ref || n_ref < 1 || !total_bytes || (c->n_alns > 0 && (!rec_size || !rec_id))) { thj_set_error("thj_span_bam_encode: bad argument"); return THJ_EINVAL; }
    return bam_encode(c, "thj_span_bam_encode", batch, tid_of_ref, n_ref, false, c->n_alns, rec_size, rec_id, nullptr, total_bytes);
}
extern "C" int thj_span_bam_encode_records(thj_ctx* c, const thj_span_batch* batch, const int32_t* tid_of_ref, int32_t n_ref, int64_t rec_cap, uint32_t* rec_size,
                                           int64_t* rec_id, int64_t* n_records, int64_t* total_bytes) {
    if (!c || !batch || !tid_of_ref || n_ref < 1 || rec_cap < 0 || !n_records || !total_bytes || (c->n_alns > 0 && (!rec_size || !rec_id))) {
        thj_set_error("thj_span_bam_encode_records: bad argument");
        return THJ_EINVAL;
    }
    return bam_encode(c, "thj_span_bam_encode_records", batch, tid_of_ref, n_ref, true, rec_cap, rec_size, rec_id, n_records, total_bytes);
}

extern "C" int thj_bam_contig_names_upload(thj_ctx* c, const char* const* names, int32_t n_ref) {
    if (!c || n_ref < 0 || (n_ref > 0 && !names)) { thj_set_error("thj_bam_contig_names_upload: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->d_contig_names) (void)hipFree(c->d_contig_names);
    if (c->d_contig_name_off) (void)hipFree(c->d_contig_name_off);
    if (c->d_contig_name_sorted) (void)hipFree(c->d_contig_name_sorted);
    c->d_contig_names = nullptr; c->d_contig_name_off = nullptr; c->d_contig_name_sorted = nullptr; c->n_contig_names = 0;
    if (n_ref == 0) return THJ_OK;
    std::vector<uint8_t> blob; std::vector<uint32_t> off{0};
    for (int32_t r = 0; r < n_ref; ++r) {
        if (!names[r]) { thj_set_error("thj_bam_contig_names_upload: contig %d has no name", (int)r + 1); return THJ_EINVAL; }
        blob.insert(blob.end(), (const uint8_t*)names[r], (const uint8_t*)names[r] + strlen(names[r]));
        if (blob.size() > 0x7FFFFFFFu) { thj_set_error("thj_bam_contig_names_upload: the names exceed 2 GiB"); return THJ_EINVAL; }
        off.push_back((uint32_t)blob.size());
    }
    HIPCHK(hipMalloc((void**)&c->d_contig_names, blob.size() + 16));
    HIPCHK(hipMalloc((void**)&c->d_contig_name_off, off.size() * 4));
    HIPCHK(hipMemcpyAsync(c->d_contig_names, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_contig_name_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    // the contigs ordered by name (bytes, then number): what a record that NAMES its contigs is looked up in by bisection (rpt::name_id)
    std::vector<uint32_t> sorted((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; ++r) sorted[(size_t)r] = (uint32_t)r;
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) {
        const size_t lx = off[x + 1] - off[x], ly = off[y + 1] - off[y];
        const int cmp = memcmp(blob.data() + off[x], blob.data() + off[y], std::min(lx, ly));
        return cmp ? cmp < 0 : lx != ly ? lx < ly : x < y;
    });
    HIPCHK(hipMalloc((void**)&c->d_contig_name_sorted, sorted.size() * 4));
    HIPCHK(hipMemcpyAsync(c->d_contig_name_sorted, sorted.data(), sorted.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->n_contig_names = n_ref;
    return THJ_OK;
}

extern "C" int thj_bam_stream_upload(thj_ctx* c, const uint8_t* bytes, int64_t n) {
    if (!c || n < 0 || (n > 0 && !bytes)) { thj_set_error("thj_bam_stream_upload: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_bam(c, (size_t)n + 64);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpyAsync(c->d_bam, bytes, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->bam_bytes = n;
    return THJ_OK;
}
extern "C" int thj_bam_stream_download(thj_ctx* c, uint8_t* bytes) {
    if (!c || (c->bam_bytes > 0 && !bytes)) { thj_set_error("thj_bam_stream_download: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (c->bam_bytes) HIPCHK(hipMemcpyAsync(bytes, c->d_bam, (size_t)c->bam_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return THJ_OK;
}

extern "C" int thj_bgzf_deflate(thj_ctx* c, int64_t n_members, const int64_t* member_end, uint8_t* comp, int64_t comp_cap, uint32_t* comp_len, uint32_t* crc,
                                int64_t* comp_bytes) {
    if (!c || n_members < 0 || (n_members > 0 && (!member_end || !comp || !comp_len || !crc)) || !comp_bytes) { thj_set_error("thj_bgzf_deflate: bad argument"); return THJ_EINVAL; }
    *comp_bytes = 0;
    if (n_members == 0) return THJ_OK;
    for (int64_t k = 0; k < n_members; ++k) {
        const int64_t b = k ? member_end[k - 1] : 0, e = member_end[k];
        if (e <= b || e - b > 65536 || e > c->bam_bytes) { thj_set_error("thj_bgzf_deflate: member %lld is empty, larger than 64 KiB or outside the encoded stream", (long long)k); return THJ_EINVAL; }
    }
    HIPCHK(hipSetDevice(c->device));
    static const int MC = getenv("THJ_DEFLATE_LAUNCH") ? atoi(getenv("THJ_DEFLATE_LAUNCH")) : 1024;       // members per launch
    const int64_t mc = n_members < MC ? n_members : (MC < 1 ? 1 : MC > 4096 ? 4096 : MC);
    // scratch: ends, then per member of a launch: tokens (256 KiB), output (64 KiB), results (16 B); the packed output
    const size_t ends_b = ((size_t)n_members * 8 + 255) & ~(size_t)255;
    const size_t need = ends_b + (size_t)mc * ((256u << 10) + (64u << 10) + 16u + (64u << 10)) + 256;
    int rc = ensure_tmp(c, need);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)c->d_bam_tmp;
    int64_t* d_ends = (int64_t*)base;
    uint32_t* d_tok = (uint32_t*)(base + ends_b);
    uint32_t* d_out = (uint32_t*)((uint8_t*)d_tok + (size_t)mc * (256u << 10));
    uint8_t* d_packed = (uint8_t*)d_out + (size_t)mc * (64u << 10);
    uint32_t* d_res = (uint32_t*)(d_packed + (size_t)mc * (64u << 10));
    HIPCHK(hipMemcpyAsync(d_ends, member_end, (size_t)n_members * 8, hipMemcpyHostToDevice, c->stream));
    std::vector<uint32_t> res((size_t)mc * 4);
    int64_t written = 0;
    for (int64_t first = 0; first < n_members; first += mc) {
        const int nm = (int)(n_members - first < mc ? n_members - first : mc);
        HIPCHK(hipMemsetAsync(d_out, 0, (size_t)nm * (64u << 10), c->stream));
        // THJ_DEFLATE_TIMING=1: the phases' durations (wall_clock64 at the phase boundaries, thread 0 of every member), mean over the launch
        static const bool timing = getenv("THJ_DEFLATE_TIMING") != nullptr;
        unsigned long long* d_tm = nullptr;
        if (timing) HIPCHK(hipMalloc((void**)&d_tm, (size_t)nm * 16 * 8));
        hipLaunchKernelGGL(thj_k_deflate, dim3((unsigned)nm), dim3(dfl::NT), 0, c->stream, (const uint8_t*)c->d_bam, (const int64_t*)d_ends, (int)first, d_tok, d_out, d_res, d_tm);
        HIPCHK(hipGetLastError());
        if (timing) {
            std::vector<unsigned long long> tm((size_t)nm * 16);
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipMemcpy(tm.data(), d_tm, tm.size() * 8, hipMemcpyDeviceToHost));
            (void)hipFree(d_tm);
            double ph[8] = {0}; unsigned long long t0 = ~0ull, t1 = 0;
            for (int m = 0; m < nm; ++m) {
                for (int k = 0; k < 8; ++k) ph[k] += (double)(tm[(size_t)m * 16 + k + 1] - tm[(size_t)m * 16 + k]);
                if (tm[(size_t)m * 16] < t0) t0 = tm[(size_t)m * 16];
                if (tm[(size_t)m * 16 + 8] > t1) t1 = tm[(size_t)m * 16 + 8];
            }
            fprintf(stderr, "[deflate] %d members, first start to last end %.1f us; mean per member (us at 100 MHz): load %.1f match %.1f totals+crc %.1f lengths %.1f crc-tree %.1f codes+header %.1f bits %.1f emit %.1f\n",
                    nm, (double)(t1 - t0) / 100.0, ph[0] / nm / 100.0, ph[1] / nm / 100.0, ph[2] / nm / 100.0, ph[3] / nm / 100.0, ph[4] / nm / 100.0, ph[5] / nm / 100.0, ph[6] / nm / 100.0, ph[7] / nm / 100.0);
        }
        hipLaunchKernelGGL(thj_k_member_offsets, dim3(1), dim3(1024), 0, c->stream, d_res, nm);
        hipLaunchKernelGGL(thj_k_pack_members, dim3((unsigned)nm), dim3(256), 0, c->stream, (const uint8_t*)d_out, (const uint32_t*)d_res, d_packed);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(res.data(), d_res, (size_t)nm * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        size_t total = 0;
        for (int m = 0; m < nm; ++m) {
            if (res[4 * (size_t)m + 2] != dfl::ST_OK) {
                thj_set_error("thj_bgzf_deflate: member %lld does not fit a BGZF block when deflated (status %u)", (long long)(first + m), res[4 * (size_t)m + 2]);
                return THJ_EFALLBACK;
            }
            comp_len[first + m] = res[4 * (size_t)m]; crc[first + m] = res[4 * (size_t)m + 1];
            total += res[4 * (size_t)m];
        }
        if (written + (int64_t)total > comp_cap) { thj_set_error("thj_bgzf_deflate: the output buffer is too small"); return THJ_EINVAL; }
        HIPCHK(hipMemcpyAsync(comp + written, d_packed, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        written += (int64_t)total;
    }
    *comp_bytes = written;
    return THJ_OK;
}

// the runtime loads a translation unit's code object at its first launch (tens of milliseconds): thj_ctx_warm makes that happen early
__global__ void thj_k_warm_bamout(int* p) { if (p) *p = 0; }
void thj_warm_bamout(hipStream_t s) { hipLaunchKernelGGL(thj_k_warm_bamout, dim3(1), dim3(64), 0, s, (int*)nullptr); }
