// rb_dev_span.hpp — the contiguous runs of the device-resident boundaries
// (rb_batch_dev.hip, rb_world_dev.hip): a block of SPAN threads moves the
// SPAN x W elements of SPAN consecutive rows of the caller's array of
// structures as one flat run, consecutive lanes on consecutive words — 16
// bytes per lane when the run's base is 16-byte aligned (VEC), else one
// element per lane (a view may start at any element) — through a tile in LDS
// with PITCH = 7 elements between rows, for both widths: lane t then reads or
// writes its row at element 7 t + d, an odd stride in elements, which spreads
// a lane group over all banks for 4- and 8-byte elements alike (the natural
// stride 6 would be 2-way conflicted).
// Included by kernel units only; everything is local to the including unit.
#pragma once
#include <stdint.h>

#include <type_traits>

namespace rb {
namespace {

constexpr int SPAN = 256;              // rows of a block, and its threads
constexpr int PITCH = 7;               // elements between two rows of a tile

// the tile element of element f of a flat run of rows of W elements
template <int W> __device__ __forceinline__ int tile_at(int f) { return W == PITCH ? f : f + f / W; }

template <typename IO, bool VEC> struct Run {
    static constexpr int V = VEC ? 16 / (int)sizeof(IO) : 1;       // elements per lane and access
    struct alignas(V * sizeof(IO)) Vec { IO v[V]; };
};

// n elements from src (rows of W) into the tile; MASKED: only the rows with row_on set are read
template <typename IO, int W, bool VEC, bool MASKED>
__device__ __forceinline__ void span_load(const IO *src, int n, IO *tile, const uint8_t *row_on) {
    using R = Run<IO, VEC>;
    const int nv = n / R::V;
    for (int i = threadIdx.x; i < nv; i += SPAN) {
        const int f = i * R::V;
        const bool first = !MASKED || row_on[f / W], last = !MASKED || row_on[(f + R::V - 1) / W];
        if (first && last) {
            const typename R::Vec x = *reinterpret_cast<const typename R::Vec *>(src + f);
#pragma unroll
            for (int j = 0; j < R::V; ++j) tile[tile_at<W>(f + j)] = x.v[j];
        } else if (first || last) {          // an access across the edge of the mask: by element
            for (int j = 0; j < R::V; ++j)
                if (row_on[(f + j) / W]) tile[tile_at<W>(f + j)] = src[f + j];
        }
    }
    for (int f = nv * R::V + threadIdx.x; f < n; f += SPAN)     // (the array's last span only)
        if (!MASKED || row_on[f / W]) tile[tile_at<W>(f)] = src[f];
}

template <typename IO, int W, bool VEC> __device__ __forceinline__ void span_store(IO *dst, int n, const IO *tile) {
    using R = Run<IO, VEC>;
    const int nv = n / R::V;
    for (int i = threadIdx.x; i < nv; i += SPAN) {
        const int f = i * R::V;
        typename R::Vec x;
#pragma unroll
        for (int j = 0; j < R::V; ++j) x.v[j] = tile[tile_at<W>(f + j)];
        *reinterpret_cast<typename R::Vec *>(dst + f) = x;
    }
    for (int f = nv * R::V + threadIdx.x; f < n; f += SPAN) dst[f] = tile[tile_at<W>(f)];
}

// the rows of the span that starts at row0 of N rows
__device__ __forceinline__ int span_rows(int64_t N, int64_t row0) { return (int)(N - row0 < SPAN ? N - row0 : SPAN); }

inline unsigned spans(int64_t N) { return (unsigned)((N + SPAN - 1) / SPAN); }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// f(std::true_type / std::false_type) by flag: a launcher's choice of a bool template argument
template <typename F> void as_flag(bool flag, F &&f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace
}  // namespace rb
