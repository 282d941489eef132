// canny_contours.hip -- outer contour chains of a finished edge map, per frame of a batch: for every kept 8-connected
// component the ordered list of its outer border pixels (the use of cv::findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE)),
// CSR-shaped on two levels.  DESIGN.md section 17.
//
// The components pipeline of canny_components.hip runs first, up to the scan: after launch_cc_resolve the entry of a
// component's FIRST pixel (its smallest r * width + c, the pixel a border follower starts from) is negative and holds the
// area; launch_cc_count + launch_points_scan give offsets[] and each row's first record number.  Then
//
//   count : one wave per image row, numbering as cc_number_kernel does (a wave prefix sum over the row's kept roots).  A
//           lane whose word holds a kept root follows that component's border once and keeps only the length: it goes
//           into chain_offsets[record + 1] for records below capacity, and the wave sums the row.  launch_points_scan
//           turns the row sums into row bases and point_offsets[].
//   place : per row, a wave prefix sum of the stored lengths onto the row base, in place: slot record + 1 held the length
//           and receives the chain's end.  A row touches only the slots of its own records, so no wave reads what another
//           one writes.
//   write : the count kernel's walk again; this time every pixel is stored at chain_offsets[record] + its position, below
//           point_capacity.
//
// Two walks per component, no counter hands out space, nothing depends on the order in which waves run: the output is
// the same bytes on every run.
//
// The walk keeps a window of 3 rows x 64 columns in six registers (three 64-bit words), centred on the pixel at which it
// was loaded; the 3 x 3 ring around the current pixel is eight bits taken from the three words, the search for the next
// border pixel one rotate and one count-leading-zeros.  A vertical step shifts the rows and loads one; the whole window is
// reloaded only when the walk comes within one column of its edge, 31 columns from where it was centred.  No table, no LDS.
// Every walk is capped at 8 * area steps: a walk is a sequence of states (pixel, search start), it ends before a state
// recurs, and there are 8 * area of them -- the cap is never reached, but no input can spin a kernel.
#include "canny_bit_walk.h" // the 3-row x 64-column walking window, shared with canny_curves.hip
#include "canny_kernels.h"

#include <algorithm>
#include <limits.h>

namespace canny {

namespace {

constexpr int kCtBlock = 256; // 4 waves: 4 image rows per workgroup step

// THE walk of the rule, from the component's first pixel (y0, x0): emit(position, pixel index) for positions 0, 1, ...
// while they lie below max_n; returns the number of positions passed (the chain's length when max_n is not reached).
template <bool BITS, class Emit>
__device__ __forceinline__ unsigned ct_trace(const void *__restrict__ src, const HystGeom &g, int row_bytes, int f, int y0,
                                             int x0, int area, unsigned long long max_n, Emit emit)
{
    if (!max_n) return 0;
    CtWalk w;
    w.y = y0, w.x = x0;
    ct_load<BITS>(w, src, g, row_bytes, f);
    const int p0 = y0 * g.width + x0;
    emit(0u, p0);
    unsigned m = ct_ring(w);
    // step 1: clockwise after W -- NW, N, NE, E, SE, S, SW
    const unsigned r1 = ((m >> 5) | (m << 3)) & 0x7Fu;
    if (!r1) return 1;
    int d = (5 + (int)__builtin_ctz(r1)) & 7;
    const int q1 = p0 + ct_dy(d) * g.width + ct_dx(d);
    int cur = p0, s = (d - 1) & 7;
    unsigned n = 1;
    const unsigned cap = 8u * (unsigned)area;
    for (unsigned step = 0; step < cap && n < max_n; step++) {
        m = ct_ring(w);
        // step 2: counter-clockwise from s -- s becomes the top bit of a byte, descending bits are descending directions
        const unsigned rot = ((m << (7 - s)) | (m >> (s + 1))) & 0xFFu;
        if (!rot) break; // cannot happen: the pixel the walk came from is set
        d = (s - ((int)__builtin_clz(rot) - 24)) & 7;
        const int nxt = cur + ct_dy(d) * g.width + ct_dx(d);
        if (nxt == p0 && cur == q1) break;
        emit(n++, nxt);
        ct_move<BITS>(w, d, src, g, row_bytes, f);
        cur = nxt;
        s = (d + 3) & 7;
    }
    return n;
}

__device__ __forceinline__ uint64_t ct_run_starts(uint64_t w) { return w & ~(w << 1); }
__device__ __forceinline__ bool ct_kept_root(int e, int min_area) { return e < 0 && (e & INT_MAX) >= min_area; }

// WRITE = false, the count: chain_offsets[record + 1] = the chain's length (records below capacity), row_points[r] = the
//   row's sum over ALL its kept roots, chain_offsets[0] = 0.
// WRITE = true: points[chain_offsets[record] + i] = the chain's i-th pixel, below point_capacity, records below capacity.
// parent is as launch_cc_resolve leaves it; row_offsets / offsets as launch_cc_count + launch_points_scan leave them.
template <bool BITS, bool WRITE>
__global__ __launch_bounds__(kCtBlock) void ct_walk_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                           const int *__restrict__ parent, int min_area,
                                                           const uint32_t *__restrict__ row_offsets,
                                                           const unsigned long long *__restrict__ offsets,
                                                           unsigned long long *chain_offsets, unsigned long long capacity,
                                                           uint32_t *__restrict__ row_points, int *__restrict__ points,
                                                           unsigned long long point_capacity)
{
    const int lane = threadIdx.x & 63;
    CT_FOR_EACH_ROW(g, r)
    {
        const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
        const int *p = parent + (size_t)f * g.height * g.width;
        unsigned run = row_offsets[r]; // kept roots of the frame before this row (wave-uniform)
        const unsigned long long frame_at = offsets[f];
        unsigned sum = 0;
        for (int k0 = 0; k0 < g.tiles_x; k0 += 64) { // rows wider than 4096 pixels take several rounds
            const int k = k0 + lane;
            const uint64_t starts = k < g.tiles_x ? ct_run_starts(ct_word<BITS>(src, g, row_bytes, f, y, k)) : 0ull;
            const int base = y * g.width + (k << 6);
            uint64_t kept = 0;
            for (uint64_t st = starts; st; st &= st - 1) {
                const int a = (int)__builtin_ctzll(st);
                if (ct_kept_root(p[base + a], min_area)) kept |= 1ull << a;
            }
            const unsigned c = (unsigned)__popcll(kept);
            unsigned incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            unsigned long long at = frame_at + run + (incl - c); // the record of this lane's first kept root
            run += __shfl(incl, 63);
            for (; kept; kept &= kept - 1, at++) {
                const int a = (int)__builtin_ctzll(kept);
                const int area = p[base + a] & INT_MAX;
                const int x0 = (k << 6) + a;
                if constexpr (!WRITE) {
                    const unsigned len = ct_trace<BITS>(src, g, row_bytes, f, y, x0, area, ~0ull, [](unsigned, int) {});
                    sum += len;
                    if (at < capacity) chain_offsets[at + 1] = len;
                } else {
                    if (at >= capacity) continue;
                    const unsigned long long begin = chain_offsets[at];
                    if (begin >= point_capacity) continue;
                    int *out = points + begin;
                    ct_trace<BITS>(src, g, row_bytes, f, y, x0, area, point_capacity - begin,
                                   [out](unsigned i, int px) { out[i] = px; });
                }
            }
        }
        if constexpr (!WRITE) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
            if (lane == 0) {
                row_points[r] = sum;
                if (r == 0 && chain_offsets) chain_offsets[0] = 0ull;
            }
        }
    }
}

// chain_offsets[record + 1]: the chain's length -> the chain's end (= the next chain's start), for records below capacity.
// row_offsets / offsets: the record CSR; row_point_offsets / point_offsets: the scan of the count kernel's row sums.
__global__ __launch_bounds__(kCtBlock) void ct_place_kernel(HystGeom g, const uint32_t *__restrict__ row_offsets,
                                                            const unsigned long long *__restrict__ offsets,
                                                            const uint32_t *__restrict__ row_point_offsets,
                                                            const unsigned long long *__restrict__ point_offsets,
                                                            unsigned long long *chain_offsets, unsigned long long capacity)
{
    const int lane = threadIdx.x & 63;
    CT_FOR_EACH_ROW(g, r)
    {
        const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
        const unsigned long long frame_at = offsets[f];
        const unsigned first = row_offsets[r];
        const unsigned past = y + 1 < g.height ? row_offsets[r + 1] : (unsigned)(offsets[f + 1] - frame_at);
        unsigned long long base = point_offsets[f] + row_point_offsets[r];
        for (unsigned i0 = first; i0 < past; i0 += 64) {
            const unsigned long long at = frame_at + i0 + lane;
            const bool mine = i0 + lane < past && at < capacity;
            unsigned long long incl = mine ? chain_offsets[at + 1] : 0ull;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (mine) chain_offsets[at + 1] = base + incl;
            base += __shfl(incl, 63);
        }
    }
}

#define CT_LAUNCH(WRITE, ...)                                                                                           \
    do {                                                                                                                \
        const unsigned grid_ = plan_ct_rows(g).grid;                                                                    \
        if (bits)                                                                                                       \
            hipLaunchKernelGGL((ct_walk_kernel<true, WRITE>), dim3(grid_), dim3(kCtBlock), 0, stream,                   \
                               (const void *)bits, g, (g.width + 7) / 8, __VA_ARGS__);                                  \
        else                                                                                                            \
            hipLaunchKernelGGL((ct_walk_kernel<false, WRITE>), dim3(grid_), dim3(kCtBlock), 0, stream,                  \
                               (const void *)strong, g, (g.width + 7) / 8, __VA_ARGS__);                                \
        return hipGetLastError();                                                                                       \
    } while (0)

} // namespace

LaunchPlan plan_ct_rows(const HystGeom &g)
{
    return capped_plan((unsigned long long)g.n_frames * g.height, kCtBlock / 64, 1u << 16);
}

hipError_t launch_ct_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *parent, int min_area,
                           const uint32_t *row_offsets, const unsigned long long *offsets,
                           unsigned long long *chain_offsets, unsigned long long capacity, uint32_t *row_points,
                           hipStream_t stream)
{
    if (!chain_offsets) capacity = 0;
    CT_LAUNCH(false, parent, min_area, row_offsets, offsets, chain_offsets, capacity, row_points, (int *)nullptr, 0ull);
}

hipError_t launch_ct_place(const HystGeom &g, const uint32_t *row_offsets, const unsigned long long *offsets,
                           const uint32_t *row_point_offsets, const unsigned long long *point_offsets,
                           unsigned long long *chain_offsets, unsigned long long capacity, hipStream_t stream)
{
    hipLaunchKernelGGL(ct_place_kernel, dim3(plan_ct_rows(g).grid), dim3(kCtBlock), 0, stream, g, row_offsets, offsets,
                       row_point_offsets, point_offsets, chain_offsets, capacity);
    return hipGetLastError();
}

hipError_t launch_ct_write(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *parent, int min_area,
                           const uint32_t *row_offsets, const unsigned long long *offsets,
                           unsigned long long *chain_offsets, unsigned long long capacity, int *points,
                           unsigned long long point_capacity, hipStream_t stream)
{
    CT_LAUNCH(true, parent, min_area, row_offsets, offsets, chain_offsets, capacity, (uint32_t *)nullptr, points,
              point_capacity);
}

} // namespace canny
