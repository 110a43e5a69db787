// thj_wave_sink.h -- the sink a WAVE writes a BAM record through (thj_accepted.hip's rewritten alignments, thj_unmapped.hip's unmapped reads).
// Records start at any byte on both sides.  The stores stay wide by aligning the DESTINATION: up to three bytes bring it to a 4-byte
// boundary, then every lane stores one aligned dword that it puts together from the two aligned source dwords its four bytes lie in
// (a funnel shift by the sides' misalignment), then up to three bytes finish; 64 lanes x 4 bytes is a full 256-byte request per
// instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "thj_accepted_core.h"

// the writing sink: one wave, every lane calls every method with the same arguments
struct WaveSink {
    uint8_t* o; uint32_t lane;
    __device__ __forceinline__ void copy(uint32_t at, const uint8_t* src, uint32_t len) {
        uint8_t* dst = o + at;
        const uint32_t head0 = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u, head = head0 < len ? head0 : len;
        if (lane < head) dst[lane] = src[lane];
        const uint32_t nd = (len - head) >> 2;
        const uint8_t* s0 = src + head;
        uint32_t* d0 = (uint32_t*)(dst + head);
        const uint32_t sh = (uint32_t)((uintptr_t)s0 & 3u) * 8u;
        // (the aligned dwords read hold at least one byte of the span each: nothing outside the allocation's dwords is touched)
        const uint32_t* sa = (const uint32_t*)((uintptr_t)s0 & ~(uintptr_t)3);
        for (uint32_t k = lane; k < nd; k += 64u) d0[k] = sh ? (sa[k] >> sh) | (sa[k + 1u] << (32u - sh)) : sa[k];
        const uint32_t done = head + 4u * nd;
        if (lane < len - done) dst[done + lane] = src[done + lane];
    }
    __device__ __forceinline__ void fill(uint32_t at, uint8_t v, uint32_t len) { for (uint32_t k = lane; k < len; k += 64u) o[at + k] = v; }
    __device__ __forceinline__ void put(uint32_t at, uint32_t v, uint32_t nbytes) { if (lane == 0u) for (uint32_t k = 0; k < nbytes; ++k) o[at + k] = (uint8_t)(v >> (8u * k)); }
    __device__ __forceinline__ void cigar(uint32_t at, const uint8_t* src, uint32_t n) {
        for (uint32_t k = lane; k < n; k += 64u) {
            const uint32_t w = acc::cigar_word(acc::rd32(src + 4u * k));
            for (uint32_t b = 0; b < 4u; ++b) o[at + 4u * k + b] = (uint8_t)(w >> (8u * b));
        }
    }
};
