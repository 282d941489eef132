// canny_fuse.hip -- temporal fusion of aligned frames and change masks: a per-pixel reduction over the time axis of a stack of
// u8 frames that honours the valid bits the warp writes (mean, lower median, min, max over windows of frames), and a per-frame
// change mask against the fused plane in the packed bit-map layout of the edge maps.  The rule is part of the interface
// (include/canny_hip.h); tests/fuse_rule.py restates it in numpy and Python ints, canny_fuse_host.cpp in
// plain C++.  All integers; every output byte has one writer; the only atomic is the integer sum behind changed[f]: the same
// bytes on every run.
//
//   One workgroup of 256 lanes per 64 x 16 output tile and trip of a capped grid.
//   A lane owns four adjacent pixels: it loads one 32-bit word per frame of the window (coalesced) and the nibble of its four
//   valid bits from the frame's bit byte, and stores one word.  The four pixels are worked on side by side in the word (SWAR)
//   or as two pairs of 16-bit lanes.
//   one pass : MEAN / MIN / MAX -- running sums (16-bit lanes: 255 * 255 fits), extremes (packed 16-bit min/max), counts (bytes).
//   registers: MEDIAN for group_len <= 8, 16, 32 -- the window is read once and kept as 16-bit lanes, an invalid sample as
//              0x100 + v so that it sorts behind every valid one; an odd-even merge sorting network of packed min/max, fully
//              unrolled (no indexed registers); the rank (c - 1) >> 1 is picked by compares.
//   passes   : MEDIAN for any group_len -- a count pass, then eight passes of a binary radix select that re-read the window.
//   mask     : one pass; two neighbouring lanes join their nibbles by a shuffle; changed[f] from wave ballots.  Here the
//              tiles of a workgroup's trips lie side by side (unit = workgroup * trips + trip), so that a wave sums the set
//              bits of a frame over its trips and adds to changed[f] once or twice, not once per tile.
#include "canny_kernels.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 16; // the warp's tile
constexpr int kPx = 4;                  // adjacent pixels of a lane: one 32-bit load per frame, one 32-bit store
constexpr unsigned kGridCap = 4096;
constexpr int kMaxRegs = 32;            // the widest register instantiation of the median
constexpr int kMeanRow = 65026;         // CANNY_HIP_FUSE_MEAN_ROW

static_assert(kTileW / kPx * kTileH == kBlock, "one lane per run of kPx pixels of the tile");

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// The mean's reciprocal: M(c) = floor((2^32 - 1) / (2c)) + 1 = ceil(2^32 / 2c), so M(c) * 2c = 2^32 + e with 0 <= e < 2c <= 510.
// For n = 2s + c <= 130305: n * e < 2^27 < 2^32, hence (n * M(c)) >> 32 = floor(n / 2c) exactly.  One division per table
// entry and workgroup, none per pixel.  M(0) = 0: a pixel without a valid sample is `fill` anyway.
__device__ __forceinline__ unsigned fz_magic(unsigned c) { return c ? 0xFFFFFFFFu / (2u * c) + 1u : 0u; }
__device__ __forceinline__ unsigned fz_mean(unsigned s, unsigned c, const unsigned *magic)
{
    return __umulhi(2u * s + c, magic[c]);
}

// nibble (MSB-first: bit 3 is pixel 0) -> one byte per pixel holding 0 or 1 (byte j is pixel j)
__device__ __forceinline__ unsigned fz_spread(unsigned nib)
{
    return ((nib * 0x01008040u) | (nib >> 3)) & 0x01010101u;
}

// What a lane knows about its run of kPx pixels in a tile.
struct FuseLane {
    size_t off;  // y * w + x
    size_t voff; // y * row_bytes + (x >> 3)
    int vshift;  // 4: the high nibble of the bit byte is this run's, 0: the low one
    int left;    // pixels of this run inside the row
    bool mine;   // the run holds at least one pixel of the plane
};

__device__ __forceinline__ FuseLane fz_lane(unsigned tx, unsigned ty, int h, int w)
{
    const int tid = threadIdx.x;
    const int x = (int)tx * kTileW + (tid & (kTileW / kPx - 1)) * kPx, y = (int)ty * kTileH + tid / (kTileW / kPx);
    FuseLane l;
    l.left = w - x;
    l.mine = y < h && l.left > 0;
    l.off = (size_t)y * w + x;
    l.voff = (size_t)y * (((size_t)w + 7) >> 3) + (x >> 3);
    l.vshift = (x & 4) ? 0 : 4;
    return l;
}

// the run's bytes packed little-endian; bytes past the row end are 0 and are never stored
__device__ __forceinline__ unsigned fz_load(const uint8_t *p, int left, int vec_ok)
{
    if (vec_ok && left >= kPx) return *(const unsigned *)p;
    unsigned v = 0;
    for (int j = 0; j < kPx && j < left; j++) v |= (unsigned)p[j] << (8 * j);
    return v;
}

__device__ __forceinline__ void fz_store(uint8_t *p, unsigned v, int left, int vec_ok)
{
    if (vec_ok && left >= kPx) {
        *(unsigned *)p = v;
    } else {
        for (int j = 0; j < kPx && j < left; j++) p[j] = (uint8_t)(v >> (8 * j));
    }
}

struct FuseArgs {
    const uint8_t *frames, *valid;
    int h, w, group_len, group_step;
    unsigned long long n_units;
    unsigned tiles_x, tiles_y;
    int fill, min_count;
    uint8_t *fused, *count;
    int vec_in, vec_out, vec_cnt; // rows of whole words from a 4-byte aligned base
};

// unit -> (plane, tile).  The 64-bit divisions cost hundreds of instructions, as much as a short window's whole work: they
// are kept for the launches that need them.
__device__ __forceinline__ void fz_unit(unsigned long long n_units, unsigned tiles_x, unsigned tiles_y, unsigned long long u,
                                        unsigned &g, unsigned &ty, unsigned &tx)
{
    if (n_units <= 0xffffffffull) { // the same on every lane
        const unsigned v = (unsigned)u, t = v / tiles_x;
        tx = v - t * tiles_x, g = t / tiles_y, ty = t - g * tiles_y;
    } else {
        const unsigned long long t = u / tiles_x;
        tx = (unsigned)(u % tiles_x), ty = (unsigned)(t % tiles_y), g = (unsigned)(t / tiles_y);
    }
}

// counts below min_count take `fill`; stores the run and its counts
__device__ __forceinline__ void fz_finish(const FuseArgs &a, unsigned g, const FuseLane &l, unsigned px, unsigned cnt)
{
    const unsigned fill = (unsigned)a.fill, mc = (unsigned)a.min_count;
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < kPx; j++) {
        const unsigned c = (cnt >> (8 * j)) & 255u, v = (px >> (8 * j)) & 255u;
        out |= (c < mc ? fill : v) << (8 * j);
    }
    const size_t at = (size_t)g * ((size_t)a.h * a.w) + l.off;
    fz_store(a.fused + at, out, l.left, a.vec_out);
    if (a.count) fz_store(a.count + at, cnt, l.left, a.vec_cnt);
}

// ---- MEAN / MIN / MAX: one pass ------------------------------------------------------------------------------------------
// kOp: 0 mean, 2 min, 3 max.  kValid: the bit maps are read; without them every sample counts.
template <int kOp, bool kValid>
__global__ __launch_bounds__(kBlock) void fuse_pass_kernel(FuseArgs a)
{
    __shared__ unsigned s_magic[256];
    if (kOp == 0) {
        s_magic[threadIdx.x] = fz_magic(threadIdx.x);
        __syncthreads();
    }
    const size_t plane = (size_t)a.h * a.w, vplane = (size_t)a.h * (((size_t)a.w + 7) >> 3);
    for (unsigned long long u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        unsigned g, ty, tx;
        fz_unit(a.n_units, a.tiles_x, a.tiles_y, u, g, ty, tx);
        const FuseLane l = fz_lane(tx, ty, a.h, a.w);
        if (!l.mine) continue;
        const size_t f0 = (size_t)g * a.group_step;
        const uint8_t *p = a.frames + f0 * plane + l.off;
        const uint8_t *pv = kValid ? a.valid + f0 * vplane + l.voff : nullptr;
        // even: pixels 0 and 2 as 16-bit lanes, odd: pixels 1 and 3
        unsigned even = kOp == 2 ? 0x00ff00ffu : 0u, odd = even, cnt = 0;
#pragma unroll 4
        for (int k = 0; k < a.group_len; k++) {
            unsigned wd = fz_load(p, l.left, a.vec_in);
            p += plane;
            if (kValid) {
                const unsigned ones = fz_spread(((unsigned)*pv >> l.vshift) & 0xfu);
                pv += vplane;
                cnt += ones;
                const unsigned m = ones * 255u;         // a byte of ones per valid pixel
                wd = kOp == 2 ? (wd | ~m) : (wd & m);   // an invalid sample: 255 for the minimum, 0 for the sum and the maximum
            }
            const unsigned e = wd & 0x00ff00ffu, o = (wd >> 8) & 0x00ff00ffu;
            if (kOp == 0)
                even += e, odd += o;                    // <= 255 * 255: no carry between the lanes
            else if (kOp == 2)
                even = pk_min(even, e), odd = pk_min(odd, o);
            else
                even = pk_max(even, e), odd = pk_max(odd, o);
        }
        if (!kValid) cnt = 0x01010101u * (unsigned)a.group_len;
        unsigned px;
        if (kOp == 0) {
            const unsigned q0 = fz_mean(even & 0xffffu, cnt & 255u, s_magic), q1 = fz_mean(odd & 0xffffu, (cnt >> 8) & 255u, s_magic);
            const unsigned q2 = fz_mean(even >> 16, (cnt >> 16) & 255u, s_magic), q3 = fz_mean(odd >> 16, cnt >> 24, s_magic);
            px = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
        } else {
            px = even | (odd << 8);
        }
        fz_finish(a, g, l, px, cnt);
    }
}

// ---- MEDIAN, registers ----------------------------------------------------------------------------------------------------
// Batcher's odd-even merge sort over K = 2^m slots: every index is a compile-time constant once the loops are unrolled.
template <int K>
__device__ __forceinline__ void fz_sort(unsigned (&e)[K], unsigned (&o)[K])
{
#pragma unroll
    for (int p = 1; p < K; p *= 2) {
#pragma unroll
        for (int k = p; k >= 1; k /= 2) {
#pragma unroll
            for (int j = k % p; j <= K - 1 - k; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < k; i++) {
                    const int lo = i + j, hi = i + j + k;
                    if (hi < K && lo / (2 * p) == hi / (2 * p)) {
                        const unsigned a0 = e[lo], b0 = e[hi], a1 = o[lo], b1 = o[hi];
                        e[lo] = pk_min(a0, b0), e[hi] = pk_max(a0, b0);
                        o[lo] = pk_min(a1, b1), o[hi] = pk_max(a1, b1);
                    }
                }
            }
        }
    }
}

template <int K, bool kValid>
__global__ __launch_bounds__(kBlock) void fuse_median_regs_kernel(FuseArgs a)
{
    const size_t plane = (size_t)a.h * a.w, vplane = (size_t)a.h * (((size_t)a.w + 7) >> 3);
    for (unsigned long long u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        unsigned g, ty, tx;
        fz_unit(a.n_units, a.tiles_x, a.tiles_y, u, g, ty, tx);
        const FuseLane l = fz_lane(tx, ty, a.h, a.w);
        if (!l.mine) continue;
        const size_t f0 = (size_t)g * a.group_step;
        const uint8_t *p = a.frames + f0 * plane + l.off;
        const uint8_t *pv = kValid ? a.valid + f0 * vplane + l.voff : nullptr;
        unsigned e[K], o[K], cnt = 0; // pixels (0, 2) and (1, 3) of every slot as 16-bit lanes
#pragma unroll
        for (int k = 0; k < K; k++) {
            // a slot behind the window re-reads the window's last frame as an invalid sample: every load is unconditional
            const bool in = k < a.group_len;
            const size_t kk = (size_t)(in ? k : a.group_len - 1);
            const unsigned wd = fz_load(p + kk * plane, l.left, a.vec_in);
            unsigned ones = kValid ? fz_spread(((unsigned)pv[kk * vplane] >> l.vshift) & 0xfu) : 0x01010101u;
            ones = in ? ones : 0u;
            cnt += ones;
            const unsigned inv = ones ^ 0x01010101u;
            e[k] = (wd & 0x00ff00ffu) | ((inv & 0x00010001u) << 8), o[k] = ((wd >> 8) & 0x00ff00ffu) | (inv & 0x01000100u);
        }
        fz_sort<K>(e, o);
        // rank (c - 1) >> 1 of each pixel, at most K / 2 - 1; a pixel with c = 0 takes slot 0 and is `fill` in the end
        const unsigned c0 = cnt & 255u, c1 = (cnt >> 8) & 255u, c2 = (cnt >> 16) & 255u, c3 = cnt >> 24;
        const unsigned r0 = (c0 - (c0 != 0)) >> 1, r1 = (c1 - (c1 != 0)) >> 1, r2 = (c2 - (c2 != 0)) >> 1, r3 = (c3 - (c3 != 0)) >> 1;
        unsigned v0 = e[0], v1 = o[0], v2 = e[0], v3 = o[0];
#pragma unroll
        for (int i = 1; i < K / 2; i++) {
            v0 = r0 == (unsigned)i ? e[i] : v0, v1 = r1 == (unsigned)i ? o[i] : v1;
            v2 = r2 == (unsigned)i ? e[i] : v2, v3 = r3 == (unsigned)i ? o[i] : v3;
        }
        const unsigned px = (v0 & 255u) | ((v1 & 255u) << 8) | (((v2 >> 16) & 255u) << 16) | (((v3 >> 16) & 255u) << 24);
        fz_finish(a, g, l, px, cnt);
    }
}

// ---- MEDIAN, passes -----------------------------------------------------------------------------------------------------
// A binary radix select per pixel, the four pixels side by side in the word.  `prefix` holds the bits decided so far (the
// lower ones 0), `rank` the rank still wanted among the valid samples that share the prefix.  Pass b counts those whose
// bit b is 0 as well: (sample ^ prefix) >> b == 0.
template <bool kValid>
__global__ __launch_bounds__(kBlock) void fuse_median_passes_kernel(FuseArgs a)
{
    const size_t plane = (size_t)a.h * a.w, vplane = (size_t)a.h * (((size_t)a.w + 7) >> 3);
    for (unsigned long long u = blockIdx.x; u < a.n_units; u += gridDim.x) {
        unsigned g, ty, tx;
        fz_unit(a.n_units, a.tiles_x, a.tiles_y, u, g, ty, tx);
        const FuseLane l = fz_lane(tx, ty, a.h, a.w);
        if (!l.mine) continue;
        const size_t f0 = (size_t)g * a.group_step;
        const uint8_t *p = a.frames + f0 * plane + l.off;
        const uint8_t *pv = kValid ? a.valid + f0 * vplane + l.voff : nullptr;
        unsigned cnt = 0x01010101u * (unsigned)a.group_len;
        if (kValid) {
            cnt = 0;
            for (int k = 0; k < a.group_len; k++) cnt += fz_spread(((unsigned)pv[(size_t)k * vplane] >> l.vshift) & 0xfu);
        }
        unsigned rank[kPx], prefix = 0;
#pragma unroll
        for (int j = 0; j < kPx; j++) {
            const unsigned c = (cnt >> (8 * j)) & 255u;
            rank[j] = (c - (c != 0)) >> 1;
        }
        for (int b = 7; b >= 0; b--) {
            const unsigned keep = 0x01010101u * (0xffu >> b); // the bits of a byte that survive >> b
            unsigned zeros = 0;                               // per pixel: samples with the prefix and bit b clear
#pragma unroll 4
            for (int k = 0; k < a.group_len; k++) {
                const unsigned wd = fz_load(p + (size_t)k * plane, l.left, a.vec_in);
                const unsigned y = ((wd ^ prefix) >> b) & keep;
                // bit 7 of a byte of nz: the byte of y is not 0
                const unsigned nz = (((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u;
                unsigned hit = (nz ^ 0x80808080u) >> 7;
                if (kValid) hit &= fz_spread(((unsigned)pv[(size_t)k * vplane] >> l.vshift) & 0xfu);
                zeros += hit;
            }
#pragma unroll
            for (int j = 0; j < kPx; j++) {
                const unsigned z = (zeros >> (8 * j)) & 255u;
                if (rank[j] >= z) rank[j] -= z, prefix |= (1u << b) << (8 * j);
            }
        }
        fz_finish(a, g, l, prefix, cnt);
    }
}

// ---- the change mask ------------------------------------------------------------------------------------------------------
struct MaskArgs {
    const uint8_t *frames, *valid, *bg, *bg_count;
    int h, w, per_bg;
    unsigned long long n_units;
    unsigned trips; // a workgroup takes the units blockIdx.x * trips .. + trips - 1: tiles side by side, one after the other
    unsigned tiles_x, tiles_y;
    int thr, min_count;
    uint8_t *mask;
    unsigned long long *changed;
    int vec_in, vec_bg, vec_cnt;
};

// A trip has three or four loads a lane and its work depends on all of them: kMaskAhead tiles are loaded before the first is
// worked on.  Measured against one tile a trip in another session only: 0.95 against 1.01 ms for 128 x 4K (DESIGN.md section
// 33); other depths were not tried.
constexpr int kMaskAhead = 4;

__global__ __launch_bounds__(kBlock) void change_mask_kernel(MaskArgs a)
{
    const size_t plane = (size_t)a.h * a.w, vplane = (size_t)a.h * (((size_t)a.w + 7) >> 3);
    // the wave's set bits of frame `cur`, not yet added to changed[cur]: a workgroup's units lie side by side, so it adds once
    // or twice per wave, not once per tile -- thousands of tiles adding to one word cost more than the whole pass
    unsigned long long acc = 0;
    unsigned cur = 0;
    for (unsigned trip = 0; trip < a.trips; trip += kMaskAhead) {
        FuseLane l[kMaskAhead];
        unsigned f[kMaskAhead], wd[kMaskAhead], bg[kMaskAhead], bc[kMaskAhead], nib[kMaskAhead];
        bool live[kMaskAhead]; // the same on every lane
#pragma unroll
        for (int i = 0; i < kMaskAhead; i++) {
            const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip + i;
            live[i] = trip + i < a.trips && u < a.n_units;
            wd[i] = bg[i] = 0, bc[i] = 0xffffffffu, nib[i] = 0, f[i] = 0;
            l[i].mine = false;
            if (!live[i]) continue;
            unsigned ty, tx;
            fz_unit(a.n_units, a.tiles_x, a.tiles_y, u, f[i], ty, tx);
            l[i] = fz_lane(tx, ty, a.h, a.w);
            if (l[i].mine) {
                const size_t b = (size_t)(f[i] / (unsigned)a.per_bg) * plane + l[i].off;
                wd[i] = fz_load(a.frames + (size_t)f[i] * plane + l[i].off, l[i].left, a.vec_in);
                bg[i] = fz_load(a.bg + b, l[i].left, a.vec_bg);
                nib[i] = a.valid ? ((unsigned)a.valid[(size_t)f[i] * vplane + l[i].voff] >> l[i].vshift) & 0xfu : 0xfu;
                if (a.bg_count) bc[i] = fz_load(a.bg_count + b, l[i].left, a.vec_cnt);
            }
        }
#pragma unroll
        for (int i = 0; i < kMaskAhead; i++) {
            if (!live[i]) break;
            unsigned bits = 0;
#pragma unroll
            for (int j = 0; j < kPx; j++) {
                const int d = (int)((wd[i] >> (8 * j)) & 255u) - (int)((bg[i] >> (8 * j)) & 255u);
                const bool on = (d < 0 ? -d : d) > a.thr && (int)((bc[i] >> (8 * j)) & 255u) >= a.min_count;
                bits |= (on ? 1u : 0u) << (kPx - 1 - j);
            }
            unsigned nb = l[i].mine ? nib[i] & bits : 0u;
            if (l[i].left < kPx) nb &= (0xfu << (kPx - (l[i].left > 0 ? l[i].left : 0))) & 0xfu; // pad bits are 0
            // uniform: every lane takes part in the exchange and in the ballots
            const unsigned other = (unsigned)__shfl_xor((int)nb, 1);
            if (l[i].mine && !(threadIdx.x & 1)) a.mask[(size_t)f[i] * vplane + l[i].voff] = (uint8_t)((nb << 4) | other);
            if (a.changed) {
                unsigned n = 0;
#pragma unroll
                for (int j = 0; j < kPx; j++) n += (unsigned)__popcll(__ballot((nb >> j) & 1u));
                if (f[i] != cur) { // the same on every lane
                    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(a.changed + cur, acc);
                    cur = f[i], acc = 0;
                }
                acc += n;
            }
        }
    }
    if (a.changed && (threadIdx.x & 63) == 0 && acc) atomicAdd(a.changed + cur, acc);
}

// canny_hip_selftest_fuse_mean: the table [255][kMeanRow]; cells with s > 255 c stay as they are
__global__ __launch_bounds__(kBlock) void fuse_mean_table_kernel(uint8_t *table)
{
    __shared__ unsigned s_magic[256];
    s_magic[threadIdx.x] = fz_magic(threadIdx.x);
    __syncthreads();
    const unsigned c = blockIdx.y + 1;
    for (unsigned s = blockIdx.x * kBlock + threadIdx.x; s <= 255u * c; s += gridDim.x * kBlock)
        table[(size_t)(c - 1) * kMeanRow + s] = (uint8_t)fz_mean(s, c, s_magic);
}

unsigned fz_tiles(int h, int w) { return (unsigned)((w + kTileW - 1) / kTileW) * (unsigned)((h + kTileH - 1) / kTileH); }

bool fz_vec(const void *p, int w) { return !(w & 3) && !((uintptr_t)p & 3); }

} // namespace

LaunchPlan plan_fuse_tiles(int n_planes, int h, int w)
{
    return capped_plan((unsigned long long)fz_tiles(h, w) * (unsigned long long)n_planes, 1, kGridCap);
}

int fuse_median_route(int group_len, int route)
{
    return group_len <= kMaxRegs && route != 2 ? 1 : 2;
}

hipError_t launch_fuse_frames(const uint8_t *frames, const uint8_t *valid, int n_frames, int h, int w, int group_len,
                              int group_step, int op, int fill, int min_count, int route, uint8_t *fused, uint8_t *count,
                              hipStream_t stream)
{
    if (!frames || !fused || n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || group_len < 1 ||
        group_len > n_frames || group_len > 255 || group_step < 1 || op < 0 || op > 3 || fill < 0 || fill > 255 ||
        min_count < 1 || min_count > 255 || route < 0 || route > 2)
        return hipErrorInvalidValue;
    const int n_groups = (n_frames - group_len) / group_step + 1;
    const LaunchPlan p = plan_fuse_tiles(n_groups, h, w);
    FuseArgs a;
    a.frames = frames, a.valid = valid, a.h = h, a.w = w, a.group_len = group_len, a.group_step = group_step;
    a.n_units = p.units, a.tiles_x = (unsigned)((w + kTileW - 1) / kTileW), a.tiles_y = (unsigned)((h + kTileH - 1) / kTileH);
    a.fill = fill, a.min_count = min_count, a.fused = fused, a.count = count;
    a.vec_in = fz_vec(frames, w), a.vec_out = fz_vec(fused, w), a.vec_cnt = fz_vec(count, w);
    const dim3 grid(p.grid), block(kBlock);
#define FUSE_LAUNCH(kernel_v, kernel_n)                                          \
    do {                                                                         \
        if (valid)                                                               \
            hipLaunchKernelGGL((kernel_v), grid, block, 0, stream, a);           \
        else                                                                     \
            hipLaunchKernelGGL((kernel_n), grid, block, 0, stream, a);           \
    } while (0)
    if (op == 0)
        FUSE_LAUNCH((fuse_pass_kernel<0, true>), (fuse_pass_kernel<0, false>));
    else if (op == 2)
        FUSE_LAUNCH((fuse_pass_kernel<2, true>), (fuse_pass_kernel<2, false>));
    else if (op == 3)
        FUSE_LAUNCH((fuse_pass_kernel<3, true>), (fuse_pass_kernel<3, false>));
    else if (fuse_median_route(group_len, route) == 2)
        FUSE_LAUNCH((fuse_median_passes_kernel<true>), (fuse_median_passes_kernel<false>));
    else if (group_len <= 8)
        FUSE_LAUNCH((fuse_median_regs_kernel<8, true>), (fuse_median_regs_kernel<8, false>));
    else if (group_len <= 16)
        FUSE_LAUNCH((fuse_median_regs_kernel<16, true>), (fuse_median_regs_kernel<16, false>));
    else
        FUSE_LAUNCH((fuse_median_regs_kernel<32, true>), (fuse_median_regs_kernel<32, false>));
#undef FUSE_LAUNCH
    return hipGetLastError();
}

hipError_t launch_change_mask(const uint8_t *frames, const uint8_t *valid, int n_frames, int h, int w, const uint8_t *bg,
                              const uint8_t *bg_count, int per_bg, int thr, int min_count, uint8_t *mask,
                              unsigned long long *changed, hipStream_t stream)
{
    if (!frames || !bg || !mask || n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || per_bg < 1 ||
        thr < 0 || thr > 255 || min_count < 1 || min_count > 255 || ((uintptr_t)changed & 7))
        return hipErrorInvalidValue;
    if (changed) {
        const hipError_t e = hipMemsetAsync(changed, 0, (size_t)n_frames * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    const LaunchPlan p = plan_fuse_tiles(n_frames, h, w);
    MaskArgs a;
    a.frames = frames, a.valid = valid, a.bg = bg, a.bg_count = bg_count, a.h = h, a.w = w, a.per_bg = per_bg;
    a.n_units = p.units, a.trips = (unsigned)p.trips(), a.tiles_x = (unsigned)((w + kTileW - 1) / kTileW), a.tiles_y = (unsigned)((h + kTileH - 1) / kTileH);
    a.thr = thr, a.min_count = min_count, a.mask = mask, a.changed = changed;
    a.vec_in = fz_vec(frames, w), a.vec_bg = fz_vec(bg, w), a.vec_cnt = fz_vec(bg_count, w);
    hipLaunchKernelGGL(change_mask_kernel, dim3(p.grid), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_fuse_mean_table(uint8_t *table, hipStream_t stream)
{
    if (!table) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(table, 0, (size_t)255 * kMeanRow, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fuse_mean_table_kernel, dim3(32, 255), dim3(kBlock), 0, stream, table);
    return hipGetLastError();
}

} // namespace canny
