// canny_components.hip -- 8-connected component labelling of a finished edge map, per frame of a batch, with per-component
// statistics and a minimum-area filter (scipy.ndimage.label with a 3x3 structure / cv::connectedComponentsWithStats(.., 8)).
// DESIGN.md section 14.
//
// The unit of work is a RUN: a maximal row of set pixels inside one 64-pixel word of the bit map (w & ~(w << 1) finds
// the run starts).  Only run STARTS carry an entry in the parent array, which is indexed by pixel (r * width + c, int) and
// lives in the caller's label plane when there is one: the array is allocated per pixel but touched per run.
//
//   link     init    : parent[s] = s for every run start s
//            merge   : every run is united with the run that continues it in the word to its left and with every run of
//                      the row above that touches it (columns a - 1 .. b + 1: the two diagonals included, also across the
//                      tile corner).  Union = find both roots, atomicMin the smaller root into the larger root's entry,
//                      retry with what was there if that entry was no root any more.  A parent is always smaller than its
//                      child, so the root of a tree is its smallest run start -- the component's first pixel in raster
//                      order -- whatever the order in which the atomics land.
//   resolve  flatten : parent[s] = root(s); a root marks itself with INT_MIN (negative = "root, area so far")
//            area    : every run adds its length to its root's entry (integer atomic add)
//   number   count   : kept roots (area >= min_area) per image row -> the scan of canny_points.hip -> offsets[] and each
//                      row's first number: the numbering is a prefix sum in raster order, no counter hands out numbers
//            number  : a kept root writes AREA and FIRST of its record and seeds the box with its own pixel; its entry
//                      becomes -k, a dropped root's INT_MIN
//            relabel : every run start replaces its entry by the final number k (0 = dropped) and folds its extent into
//                      the record's box (atomicMin / atomicMax); fixup turns right / bottom into WIDTH / HEIGHT
//   write            : one wave per tile row by row: every pixel takes the entry of its run's start -> labels (full rows,
//                      zeros included, 256 contiguous bytes per store) and kept_u8
//
// Every access to the parent array inside a launch in which another workgroup may write the same word is an agent-scope
// atomic (relaxed): the per-CU L1 and the per-XCD L2 are not kept coherent for plain accesses.  Kernel boundaries order
// the phases.  No iteration count depends on the host: a launch sequence is fixed by which outputs were asked for.
//
// Two sources, as canny_points.hip: the converged strong bit-plane (tile-major) or a caller's packed bit map (rows
// MSB-first, padded to bytes, any byte address; padding bits masked off).
#include "canny_kernels.h"

#include <algorithm>
#include <limits.h>

namespace canny {

namespace {

constexpr int kCcBlock = 256; // 4 waves: 4 tiles (tile kernels) or 4 image rows (row kernels) per workgroup step
constexpr int kRootMark = INT_MIN;

__device__ __forceinline__ int cc_ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_st(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_min(int *p, int v)
{
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cc_max(int *p, int v)
{
    return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cc_add(int *p, int v)
{
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// columns 64*k .. 64*k + 63 of row y of frame f, bit i = column 64*k + i; rows and words outside the frame and columns
// >= width read as 0
template <bool BITS>
__device__ __forceinline__ uint64_t cc_word(const void *__restrict__ src, const HystGeom &g, int row_bytes, int f, int y,
                                            int k)
{
    if (y < 0 || y >= g.height || k < 0 || k >= g.tiles_x) return 0ull;
    return row_word<BITS>(src, g, row_bytes, f, y, k);
}

__device__ __forceinline__ uint64_t run_starts(uint64_t w) { return w & ~(w << 1); }
// length of the run of ones that starts at bit a of w (bit a set)
__device__ __forceinline__ int run_len(uint64_t w, int a)
{
    const uint64_t rest = ~(w >> a);
    return rest ? (int)__builtin_ctzll(rest) : 64; // 64: a == 0 and the word is all ones
}
// number of ones at the top of w (bit 63 downwards)
__device__ __forceinline__ int top_ones(uint64_t w) { return ~w ? (int)__builtin_clzll(~w) : 64; }
__device__ __forceinline__ uint64_t bits_below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); } // bits 0 .. n - 1

// merge phase only: no entry is negative yet
__device__ __forceinline__ int cc_find(const int *p, int x)
{
    for (;;) {
        const int v = cc_ld(p + x);
        if (v == x) return x;
        x = v;
    }
}

// Unites the trees of a and b; returns the root they share afterwards (at the moment of the link).
__device__ __forceinline__ int cc_union(int *p, int a, int b)
{
    for (;;) {
        a = cc_find(p, a);
        b = cc_find(p, b);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = cc_min(p + a, b); // a > b: hang a below b, if a is still a root
        if (old == a) return b;
        a = old; // a had a parent already (now min(old, b)): its former parent and b remain to be united
    }
}

struct TileAt {
    int f, ty, tx;
};
__device__ __forceinline__ TileAt tile_at(const HystGeom &g, int tile)
{
    TileAt t;
    const int per_frame = g.tiles_x * g.tiles_y;
    t.f = tile / per_frame;
    const int r = tile - t.f * per_frame;
    t.ty = r / g.tiles_x;
    t.tx = r - t.ty * g.tiles_x;
    return t;
}

#define CC_FOR_EACH_TILE(g, tile)                                                                                       \
    for (int tile = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_tiles_ = (g).tiles(),                        \
             stride_ = (int)((gridDim.x * blockDim.x) >> 6);                                                            \
         tile < n_tiles_; tile += stride_)

// ---- link ------------------------------------------------------------------------------------------------------------
template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                           int *__restrict__ parent)
{
    const int lane = threadIdx.x & 63;
    const size_t frame_px = (size_t)g.height * g.width;
    CC_FOR_EACH_TILE(g, tile)
    {
        const TileAt t = tile_at(g, tile);
        const int y = t.ty * kTile + lane;
        uint64_t st = run_starts(cc_word<BITS>(src, g, row_bytes, t.f, y, t.tx));
        int *p = parent + (size_t)t.f * frame_px;
        const int base = y * g.width + t.tx * kTile;
        while (st) {
            const int s = base + (int)__builtin_ctzll(st);
            p[s] = s;
            st &= st - 1;
        }
    }
}

template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_merge_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                            int *parent)
{
    const int lane = threadIdx.x & 63;
    const size_t frame_px = (size_t)g.height * g.width;
    CC_FOR_EACH_TILE(g, tile)
    {
        const TileAt t = tile_at(g, tile);
        const int y = t.ty * kTile + lane;
        const uint64_t w = cc_word<BITS>(src, g, row_bytes, t.f, y, t.tx);
        if (!w) continue;
        int *p = parent + (size_t)t.f * frame_px;
        const uint64_t up = cc_word<BITS>(src, g, row_bytes, t.f, y - 1, t.tx);
        const uint64_t left = cc_word<BITS>(src, g, row_bytes, t.f, y, t.tx - 1);
        const uint64_t up_left = cc_word<BITS>(src, g, row_bytes, t.f, y - 1, t.tx - 1);
        const uint64_t up_right = cc_word<BITS>(src, g, row_bytes, t.f, y - 1, t.tx + 1);
        const int base = y * g.width + t.tx * kTile, up_base = base - g.width;
        uint64_t st = run_starts(w);
        while (st) {
            const int a = (int)__builtin_ctzll(st);
            st &= st - 1;
            const int b = a + run_len(w, a) - 1;
            const int s = base + a;
            int root = s;
            // the run continues one that ends the word to the left
            if (a == 0 && (left >> 63)) root = cc_union(p, s, base - top_ones(left));
            // runs of the row above that touch columns a - 1 .. b + 1
            uint64_t touch = up & bits_below(min(b + 2, 64)) & ~bits_below(max(a - 1, 0));
            while (touch) {
                const int bit = (int)__builtin_ctzll(touch);
                const uint64_t gaps = ~up & bits_below(bit);
                const int first = gaps ? 64 - (int)__builtin_clzll(gaps) : 0; // where the run holding `bit` starts
                root = cc_union(p, s, up_base + first);
                touch &= ~bits_below(bit + run_len(up, bit));
            }
            if (a == 0 && (up_left >> 63)) root = cc_union(p, s, up_base - top_ones(up_left));
            if (b == 63 && (up_right & 1ull)) root = cc_union(p, s, up_base + kTile);
            if (root < s) cc_min(p + s, root); // shortcut: root is an ancestor of s (or becomes its parent)
        }
    }
}

// ---- resolve ---------------------------------------------------------------------------------------------------------
template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_flatten_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                              int *parent)
{
    const int lane = threadIdx.x & 63;
    const size_t frame_px = (size_t)g.height * g.width;
    CC_FOR_EACH_TILE(g, tile)
    {
        const TileAt t = tile_at(g, tile);
        const int y = t.ty * kTile + lane;
        uint64_t st = run_starts(cc_word<BITS>(src, g, row_bytes, t.f, y, t.tx));
        int *p = parent + (size_t)t.f * frame_px;
        const int base = y * g.width + t.tx * kTile;
        while (st) {
            const int s = base + (int)__builtin_ctzll(st);
            st &= st - 1;
            int x = s;
            for (;;) { // a root reads as itself or, once it has marked itself, as a negative word
                const int v = cc_ld(p + x);
                if (v < 0 || v == x) break;
                x = v;
            }
            cc_st(p + s, x == s ? kRootMark : x);
        }
    }
}

template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_area_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                           int *parent)
{
    const int lane = threadIdx.x & 63;
    const size_t frame_px = (size_t)g.height * g.width;
    CC_FOR_EACH_TILE(g, tile)
    {
        const TileAt t = tile_at(g, tile);
        const int y = t.ty * kTile + lane;
        const uint64_t w = cc_word<BITS>(src, g, row_bytes, t.f, y, t.tx);
        uint64_t st = run_starts(w);
        int *p = parent + (size_t)t.f * frame_px;
        const int base = y * g.width + t.tx * kTile;
        while (st) {
            const int a = (int)__builtin_ctzll(st);
            st &= st - 1;
            const int s = base + a;
            const int e = cc_ld(p + s); // a root's own entry stays negative whatever has been added: area < 2^31
            cc_add(p + (e < 0 ? s : e), run_len(w, a));
        }
    }
}

// ---- number ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool entry_is_kept_root(int e, int min_area) { return e < 0 && (e & INT_MAX) >= min_area; }

#define CC_FOR_EACH_ROW(g, r)                                                                                           \
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_rows_ = (size_t)(g).n_frames * (g).height,  \
                stride_ = ((size_t)gridDim.x * blockDim.x) >> 6;                                                        \
         r < n_rows_; r += stride_)

template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_count_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                            const int *__restrict__ parent, int min_area,
                                                            uint32_t *__restrict__ row_counts)
{
    const int lane = threadIdx.x & 63;
    CC_FOR_EACH_ROW(g, r)
    {
        const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
        const int *p = parent + (size_t)f * g.height * g.width;
        unsigned c = 0;
        for (int k = lane; k < g.tiles_x; k += 64) {
            uint64_t st = run_starts(cc_word<BITS>(src, g, row_bytes, f, y, k));
            const int base = y * g.width + (k << 6);
            while (st) {
                c += entry_is_kept_root(p[base + (int)__builtin_ctzll(st)], min_area) ? 1u : 0u;
                st &= st - 1;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) row_counts[r] = c;
    }
}

// Roots get their final entry (-k kept, INT_MIN dropped); the records of kept roots below capacity are seeded.
template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_number_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                             int *__restrict__ parent, int min_area,
                                                             const uint32_t *__restrict__ row_offsets,
                                                             const unsigned long long *__restrict__ offsets,
                                                             int *__restrict__ stats, unsigned long long capacity)
{
    const int lane = threadIdx.x & 63;
    CC_FOR_EACH_ROW(g, r)
    {
        const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
        int *p = parent + (size_t)f * g.height * g.width;
        unsigned run = row_offsets[r]; // kept roots of the frame before this row (wave-uniform)
        const unsigned long long frame_at = offsets[f];
        for (int k0 = 0; k0 < g.tiles_x; k0 += 64) { // rows wider than 4096 pixels take several rounds
            const int k = k0 + lane;
            const uint64_t starts = k < g.tiles_x ? run_starts(cc_word<BITS>(src, g, row_bytes, f, y, k)) : 0ull;
            const int base = y * g.width + (k << 6);
            uint64_t roots = 0, kept = 0;
            for (uint64_t st = starts; st; st &= st - 1) {
                const int a = (int)__builtin_ctzll(st);
                const int e = p[base + a];
                if (e < 0) roots |= 1ull << a;
                if (entry_is_kept_root(e, min_area)) kept |= 1ull << a;
            }
            const unsigned c = (unsigned)__popcll(kept);
            unsigned incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            unsigned number = run + (incl - c); // numbers are 1-based: the first kept root of this lane gets number + 1
            run += __shfl(incl, 63);
            for (; roots; roots &= roots - 1) {
                const int a = (int)__builtin_ctzll(roots);
                const int s = base + a;
                if (!(kept >> a & 1ull)) {
                    p[s] = kRootMark;
                    continue;
                }
                const int area = p[s] & INT_MAX;
                number++;
                const unsigned long long at = frame_at + number - 1;
                if (stats && at < capacity) {
                    int *rec = stats + at * 6;
                    const int x = (k << 6) + a;
                    rec[0] = x, rec[1] = y, rec[2] = x, rec[3] = y; // LEFT, TOP, right, bottom (fixup: WIDTH, HEIGHT)
                    rec[4] = area, rec[5] = s;
                }
                p[s] = -(int)number;
            }
        }
    }
}

__device__ __forceinline__ int number_of_root_entry(int v) { return v >= 0 ? v : (v == kRootMark ? 0 : -v); }

// Every run start's entry becomes its component's number; the run's extent goes into the record's box.
template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_relabel_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                              int *parent, const unsigned long long *__restrict__ offsets,
                                                              int *stats, unsigned long long capacity)
{
    const int lane = threadIdx.x & 63;
    const size_t frame_px = (size_t)g.height * g.width;
    CC_FOR_EACH_TILE(g, tile)
    {
        const TileAt t = tile_at(g, tile);
        const int y = t.ty * kTile + lane;
        const uint64_t w = cc_word<BITS>(src, g, row_bytes, t.f, y, t.tx);
        if (!w) continue;
        int *p = parent + (size_t)t.f * frame_px;
        const int base = y * g.width + t.tx * kTile;
        const unsigned long long frame_at = offsets[t.f];
        for (uint64_t st = run_starts(w); st; st &= st - 1) {
            const int a = (int)__builtin_ctzll(st);
            const int s = base + a;
            const int e = cc_ld(p + s); // own entry: negative = root (nobody else writes it), else the root's index
            // a root's entry is -k / INT_MIN until the root itself has replaced it by k / 0: both read as k
            const int k = number_of_root_entry(e < 0 ? e : cc_ld(p + e));
            if (k > 0 && stats) {
                const unsigned long long at = frame_at + (unsigned)k - 1;
                if (at < capacity) {
                    int *rec = stats + at * 6;
                    const int x0 = t.tx * kTile + a, x1 = x0 + run_len(w, a) - 1;
                    cc_min(rec + 0, x0);
                    cc_max(rec + 2, x1);
                    cc_max(rec + 3, y);
                }
            }
            cc_st(p + s, k);
        }
    }
}

__global__ __launch_bounds__(256) void cc_fixup_kernel(int *__restrict__ stats,
                                                       const unsigned long long *__restrict__ offsets, int n_frames,
                                                       unsigned long long capacity)
{
    const unsigned long long n = min(offsets[n_frames], capacity);
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        int *rec = stats + i * 6;
        rec[2] = rec[2] - rec[0] + 1;
        rec[3] = rec[3] - rec[1] + 1;
    }
}

// ---- write -----------------------------------------------------------------------------------------------------------
// entries may be the label plane itself: a wave reads the entries of a row's run starts, then stores the row (the entry of
// a run start is rewritten with the value it holds); no other wave reads or writes these 64 pixels
template <bool BITS>
__global__ __launch_bounds__(kCcBlock) void cc_write_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                            const int *entries, int *labels, uint8_t *__restrict__ kept)
{
    const int lane = threadIdx.x & 63;
    const size_t frame_px = (size_t)g.height * g.width;
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull); // bits 0 .. lane
    CC_FOR_EACH_TILE(g, tile)
    {
        const TileAt t = tile_at(g, tile);
        const uint64_t mine = cc_word<BITS>(src, g, row_bytes, t.f, t.ty * kTile + lane, t.tx);
        const int x = t.tx * kTile + lane;
        const int rows = min(kTile, g.height - t.ty * kTile);
        for (int i = 0; i < rows; i++) {
            const uint64_t w = __shfl(mine, i);
            const size_t row_at = (size_t)t.f * frame_px + (size_t)(t.ty * kTile + i) * g.width;
            int v = 0;
            if (w >> lane & 1ull) {
                const int start = 63 - (int)__builtin_clzll(run_starts(w) & upto);
                v = entries[row_at + t.tx * kTile + start];
            }
            if (x < g.width) {
                if (labels) labels[row_at + x] = v;
                if (kept) kept[row_at + x] = v ? 255 : 0;
            }
        }
    }
}

#define CC_LAUNCH(kernel, grid, ...)                                                                                    \
    do {                                                                                                                \
        if (bits)                                                                                                       \
            hipLaunchKernelGGL(kernel<true>, dim3(grid), dim3(kCcBlock), 0, stream, (const void *)bits, g,              \
                               (g.width + 7) / 8, __VA_ARGS__);                                                         \
        else                                                                                                            \
            hipLaunchKernelGGL(kernel<false>, dim3(grid), dim3(kCcBlock), 0, stream, (const void *)strong, g,           \
                               (g.width + 7) / 8, __VA_ARGS__);                                                         \
        const hipError_t e_ = hipGetLastError();                                                                        \
        if (e_ != hipSuccess) return e_;                                                                                \
    } while (0)

} // namespace

LaunchPlan plan_cc_tiles(const HystGeom &g)
{
    return capped_plan((unsigned long long)g.tiles(), kCcBlock / 64, 1u << 16);
}
LaunchPlan plan_cc_rows(const HystGeom &g)
{
    return capped_plan((unsigned long long)g.n_frames * g.height, kCcBlock / 64, 1u << 16);
}
LaunchPlan plan_cc_fixup(unsigned long long capacity) { return capped_plan(capacity, 256, 4096); }

hipError_t launch_cc_link(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int *parent, hipStream_t stream)
{
    CC_LAUNCH(cc_init_kernel, plan_cc_tiles(g).grid, parent);
    CC_LAUNCH(cc_merge_kernel, plan_cc_tiles(g).grid, parent);
    return hipSuccess;
}

hipError_t launch_cc_resolve(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int *parent,
                             hipStream_t stream)
{
    CC_LAUNCH(cc_flatten_kernel, plan_cc_tiles(g).grid, parent);
    CC_LAUNCH(cc_area_kernel, plan_cc_tiles(g).grid, parent);
    return hipSuccess;
}

hipError_t launch_cc_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *parent, int min_area,
                           uint32_t *row_counts, hipStream_t stream)
{
    CC_LAUNCH(cc_count_kernel, plan_cc_rows(g).grid, parent, min_area, row_counts);
    return hipSuccess;
}

hipError_t launch_cc_number(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int *parent, int min_area,
                            const uint32_t *row_offsets, const unsigned long long *offsets, int *stats,
                            unsigned long long capacity, hipStream_t stream)
{
    if (!capacity) stats = nullptr;
    CC_LAUNCH(cc_number_kernel, plan_cc_rows(g).grid, parent, min_area, row_offsets, offsets, stats, capacity);
    CC_LAUNCH(cc_relabel_kernel, plan_cc_tiles(g).grid, parent, offsets, stats, capacity);
    if (stats) {
        hipLaunchKernelGGL(cc_fixup_kernel, dim3(plan_cc_fixup(capacity).grid), dim3(256), 0, stream, stats, offsets,
                           g.n_frames, capacity);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_cc_write(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *entries, int *labels,
                           uint8_t *kept, hipStream_t stream)
{
    CC_LAUNCH(cc_write_kernel, plan_cc_tiles(g).grid, entries, labels, kept);
    return hipSuccess;
}

} // namespace canny
