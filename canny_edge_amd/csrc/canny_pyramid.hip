// canny_pyramid.hip -- image pyramids of u8 planes: pyrDown (the 5 x 5 binomial (1 4 6 4 1)^2 with reflect-101 borders, every
// second row and column, (s + 128) >> 8) and pyrUp (the same kernel on the zero-inserted grid, (s + 32) >> 6).  The rule is
// part of the interface (include/canny_hip.h); tests/pyramid_rule.py restates it in numpy,
// canny_pyramid_host.cpp pixel by pixel in plain C++.  All integers; every output byte has one writer; no atomics: the same
// bytes on every run and route.
//
//   Every launch walks tiles of 128 columns x 32 rows of its OUTPUT, one per workgroup of 256 lanes and trip of a capped grid.
//   direct   : (route 1, the cross-check) a lane per output pixel, 25 taps from global memory, every index folded.
//   tiled    : (route 2) the filter separated.  Horizontal pass: a wave takes a source row of the tile's footprint (2 th + 3
//              rows of 259 columns); a lane loads ONE word of four source bytes, takes its neighbours' words by cross-lane
//              moves (the two halo words of a row are loaded by lanes 0 and 63), and forms two decimated partial sums, each at
//              most 4080, as the two 16-bit halves of one LDS word: [67][64] words, 17 KB.  Vertical pass: a lane owns four
//              adjacent output pixels (two LDS words, one 64-bit read a row) of four output rows and runs the five taps on the
//              packed halves: at most 65280 + 128, no carry between the halves.  It stores one word where the four pixels
//              exist and the address is 4-byte aligned, bytes otherwise.
//              A tile whose footprint lies inside the frame, on a u8 plane whose rows start on word addresses, loads with no
//              test at all (a workgroup-uniform branch); every other tile folds the indices of each byte it reads, and still
//              loads whole words where a lane's four bytes lie in the row and on a word address.
//   pyrUp    : a lane produces two blocks of 4 columns x 2 rows from their 3 x 4 source neighbourhoods: per source row the
//              four horizontal sums as packed halves (at most 2040), shared by the two output rows; a word store where aligned.
#include "canny_kernels.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 128, kTH = 32;      // output tile: columns x rows
constexpr int kSrcRows = 2 * kTH + 3;   // source rows under a tile
constexpr int kRowWords = kTW / 2;      // LDS words of a row of partial sums: two 16-bit sums each
constexpr int kWaves = kBlock / 64;
constexpr int kRowsPerWave = (kSrcRows + kWaves - 1) / kWaves;
constexpr unsigned kGridCap = 4096;
constexpr unsigned kEven = 0x00FF00FFu;

static_assert(kRowWords == 64, "a wave takes a source row: one word of four source bytes a lane");
static_assert((kTW / 4) * (kTH / 4) == kBlock, "the vertical pass: a lane per four pixels of four rows");
static_assert((kTW / 4) * (kTH / 2) == 2 * kBlock, "pyrUp: a lane per two blocks of four pixels of two rows");

struct PyrArgs {
    const void *src;
    uint8_t *dst;
    int h, w, oh, ow; // source and output planes
    unsigned long long n_units;
    unsigned trips, tiles_x, tiles_y;
    int src_s16; // a plane of shorts in [0, 255] (the context's smoothed plane) instead of bytes
};

struct Tile {
    unsigned f;
    int x0, y0, tw, th; // the output tile: origin and the columns and rows that exist
};

__device__ __forceinline__ Tile tile_of(const PyrArgs &a, unsigned long long u)
{
    const unsigned per_frame = a.tiles_x * a.tiles_y;
    const unsigned f = (unsigned)(u / per_frame), t = (unsigned)(u % per_frame);
    Tile tl;
    tl.f = f, tl.x0 = (int)(t % a.tiles_x) * kTW, tl.y0 = (int)(t / a.tiles_x) * kTH;
    tl.tw = min(kTW, a.ow - tl.x0), tl.th = min(kTH, a.oh - tl.y0);
    return tl;
}

// reflect-101
__device__ __forceinline__ int fold(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

__device__ __forceinline__ unsigned load_px(const void *p, int s16, size_t i)
{
    return s16 ? (unsigned)static_cast<const uint16_t *>(p)[i] & 0xFFu : (unsigned)static_cast<const uint8_t *>(p)[i];
}

// the four bytes that start `shift` (0..3) bytes into lo, continued in hi
__device__ __forceinline__ unsigned bytes_at(unsigned lo, unsigned hi, int shift)
{
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)shift);
}

// four output pixels (lo: pixels 0 and 1, hi: pixels 2 and 3, a byte in each 16-bit half) at dst[idx .. idx + nv - 1]
__device__ __forceinline__ void store_four(uint8_t *dst, size_t idx, int nv, unsigned lo, unsigned hi)
{
    const unsigned v = (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi >> 16) << 24);
    uint8_t *d = dst + idx;
    if (nv >= 4 && !((uintptr_t)d & 3)) {
        *reinterpret_cast<unsigned *>(d) = v;
    } else {
        for (int j = 0; j < min(nv, 4); j++) d[j] = (uint8_t)(v >> (8 * j));
    }
}

// ---- pyrDown, route 1: the rule as it is written ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pyr_down_direct_kernel(PyrArgs a)
{
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break;
        const Tile tl = tile_of(a, u);
        const size_t in_base = (size_t)tl.f * (size_t)a.h * (size_t)a.w, out_base = (size_t)tl.f * (size_t)a.oh * (size_t)a.ow;
        for (int i = threadIdx.x; i < kTW * kTH; i += kBlock) {
            const int lx = i % kTW, ly = i / kTW;
            if (lx >= tl.tw || ly >= tl.th) continue;
            const int x = tl.x0 + lx, y = tl.y0 + ly;
            unsigned s = 0;
            for (int j = 0; j < 5; j++) {
                const size_t row = in_base + (size_t)fold(2 * y + j - 2, a.h) * (size_t)a.w;
                const unsigned kj = j == 2 ? 6u : ((j & 1) ? 4u : 1u);
                unsigned r = 0;
                for (int k = 0; k < 5; k++) {
                    const unsigned kk = k == 2 ? 6u : ((k & 1) ? 4u : 1u);
                    r += kk * load_px(a.src, a.src_s16, row + (size_t)fold(2 * x + k - 2, a.w));
                }
                s += kj * r;
            }
            a.dst[out_base + (size_t)y * (size_t)a.ow + (size_t)x] = (uint8_t)((s + 128u) >> 8);
        }
    }
}

// ---- pyrDown, route 2: separated, packed, through LDS -------------------------------------------------------------------------
// A word of four source columns as a border tile reads it: the columns gx .. gx + 3, each folded into [0, w) once per tile.
struct FoldedWord {
    int gx, col[4];
    bool straight; // the four columns lie in the row as they are: one word load where the address allows
};

__device__ __forceinline__ FoldedWord folded_word(const PyrArgs &a, int gx)
{
    FoldedWord fw;
    fw.gx = gx, fw.straight = !a.src_s16 && gx >= 0 && gx + 3 < a.w;
#pragma unroll
    for (int j = 0; j < 4; j++) fw.col[j] = fold(gx + j, a.w);
    return fw;
}

// row: the element offset of the source row
__device__ __forceinline__ unsigned load_folded(const PyrArgs &a, size_t row, const FoldedWord &fw)
{
    if (fw.straight) {
        const uint8_t *p = static_cast<const uint8_t *>(a.src) + row + fw.gx;
        if (!((uintptr_t)p & 3)) return *reinterpret_cast<const unsigned *>(p);
    }
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) v |= load_px(a.src, a.src_s16, row + (size_t)fw.col[j]) << (8 * j);
    return v;
}

// The two partial sums of a lane: `own` holds the source columns c .. c + 3 (c = 2 * the lane's first output column), left
// the four before and right the four after.  Low half: the output centred on c, high half: the one centred on c + 2.
__device__ __forceinline__ unsigned row_sums(unsigned left, unsigned own, unsigned right)
{
    const unsigned lo = bytes_at(left, own, 2), hi = bytes_at(own, right, 2); // columns c - 2 .. c + 1 and c + 2 .. c + 5
    const unsigned t0 = lo & kEven, t1 = (lo >> 8) & kEven, t2 = own & kEven, t3 = (own >> 8) & kEven, t4 = hi & kEven;
    return t0 + t4 + 4u * (t1 + t3) + 6u * t2;
}

// A wave's row of partial sums from its 64 words and the two halo words, the left one held by lane 0 and the right one by
// lane 63; every lane of the wave calls.  The neighbours' words come by the wavefront shifts of the DPP modifier (wave_shr:1 =
// 0x138: lane i takes lane i - 1; wave_shl:1 = 0x130: lane i takes lane i + 1), which leave the end lane with the first
// operand -- its halo word: no LDS round trip, no select.
__device__ __forceinline__ void put_row(unsigned *s_row, int lane, unsigned own, unsigned halo)
{
    const unsigned left = (unsigned)__builtin_amdgcn_update_dpp((int)halo, (int)own, 0x138, 0xF, 0xF, false);
    const unsigned right = (unsigned)__builtin_amdgcn_update_dpp((int)halo, (int)own, 0x130, 0xF, 0xF, false);
    s_row[lane] = row_sums(left, own, right);
}

// The footprint's rows sy = wave, wave + 4, .. < 2 th + 3 (frame rows 2 y0 - 2 + sy); lane k loads the word of the columns
// 2 x0 + 4 k .., lanes 0 and 63 also the row's halo words: the columns 2 x0 - 4 .. and 2 x0 + 256 ..
// INSIDE: the footprint lies inside the frame, the plane is bytes and every row starts on a word address
__device__ __forceinline__ void horizontal_pass_inside(const PyrArgs &a, const Tile &tl, unsigned *s_sum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_rows = 2 * tl.th + 3;
    const uint8_t *p = static_cast<const uint8_t *>(a.src) + (size_t)tl.f * (size_t)a.h * (size_t)a.w +
                       (size_t)(2 * tl.y0 - 2 + wave) * (size_t)a.w + 2 * tl.x0;
    const int own_at = 4 * lane, halo_at = lane == 0 ? -4 : 2 * kTW;
    const size_t step = (size_t)kWaves * (size_t)a.w;
    unsigned own[kRowsPerWave], halo[kRowsPerWave];
    // all loads of the wave first: 17 words a lane in flight
#pragma unroll
    for (int i = 0; i < kRowsPerWave; i++) {
        own[i] = halo[i] = 0;
        if (wave + kWaves * i >= n_rows) continue; // the same on every lane of the wave
        own[i] = *reinterpret_cast<const unsigned *>(p + i * step + own_at);
        if (lane == 0 || lane == 63) halo[i] = *reinterpret_cast<const unsigned *>(p + i * step + halo_at);
    }
#pragma unroll
    for (int i = 0; i < kRowsPerWave; i++) {
        const int sy = wave + kWaves * i;
        if (sy < n_rows) put_row(s_sum + sy * kRowWords, lane, own[i], halo[i]);
    }
}

// every other tile: the rows and columns folded, row by row
__device__ __forceinline__ void horizontal_pass_border(const PyrArgs &a, const Tile &tl, unsigned *s_sum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_rows = 2 * tl.th + 3;
    const size_t base = (size_t)tl.f * (size_t)a.h * (size_t)a.w;
    // a lane whose word no existing output reads loads nothing (its folds could run long on a narrow plane)
    const bool wanted = 2 * lane <= tl.tw, halo_wanted = lane == 0 || (lane == 63 && tl.tw == kTW);
    FoldedWord own_w{}, halo_w{};
    if (wanted) own_w = folded_word(a, 2 * tl.x0 + 4 * lane);
    if (halo_wanted) halo_w = folded_word(a, 2 * tl.x0 + (lane == 0 ? -4 : 2 * kTW));
#pragma unroll 1
    for (int sy = wave; sy < n_rows; sy += kWaves) {
        const size_t row = base + (size_t)fold(2 * tl.y0 - 2 + sy, a.h) * (size_t)a.w;
        const unsigned own = wanted ? load_folded(a, row, own_w) : 0u;
        const unsigned halo = halo_wanted ? load_folded(a, row, halo_w) : 0u;
        put_row(s_sum + sy * kRowWords, lane, own, halo);
    }
}

__global__ __launch_bounds__(kBlock) void pyr_down_tiled_kernel(PyrArgs a)
{
    __shared__ __attribute__((aligned(8))) unsigned s_sum[kSrcRows * kRowWords];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const bool rows_on_words = !a.src_s16 && !((uintptr_t)a.src & 3) && !(a.w & 3);
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const Tile tl = tile_of(a, u);
        __syncthreads(); // the last trip has read its LDS
        // the footprint: rows 2 y0 - 2 .. 2 y0 + 2 th, columns 2 x0 - 4 .. 2 x0 + 259 as whole words
        const bool inside = rows_on_words && tl.tw == kTW && tl.y0 > 0 && 2 * tl.y0 + 2 * tl.th < a.h && tl.x0 > 0 &&
                            2 * tl.x0 + 2 * kTW + 3 < a.w;
        if (inside)
            horizontal_pass_inside(a, tl, s_sum);
        else
            horizontal_pass_border(a, tl, s_sum);
        __syncthreads();
        const int x = tl.x0 + 4 * lx;
        if (x >= a.ow) continue;
        const int nv = a.ow - x;
        const size_t out_base = (size_t)tl.f * (size_t)a.oh * (size_t)a.ow;
        const uint2 *col = reinterpret_cast<const uint2 *>(s_sum) + lx;
        uint2 r[11]; // the partial sums under the lane's four output rows: rows 8 ly .. 8 ly + 10 of the footprint
#pragma unroll
        for (int j = 0; j < 11; j++) r[j] = 8 * ly + j < 2 * tl.th + 3 ? col[(8 * ly + j) * (kRowWords / 2)] : make_uint2(0u, 0u);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int oy = 4 * ly + q;
            if (oy >= tl.th) break;
            const uint2 *p = r + 2 * q;
            const unsigned lo = p[0].x + p[4].x + 4u * (p[1].x + p[3].x) + 6u * p[2].x + 0x00800080u;
            const unsigned hi = p[0].y + p[4].y + 4u * (p[1].y + p[3].y) + 6u * p[2].y + 0x00800080u;
            store_four(a.dst, out_base + (size_t)(tl.y0 + oy) * (size_t)a.ow + (size_t)x, nv, (lo >> 8) & kEven, (hi >> 8) & kEven);
        }
    }
}

// ---- pyrUp ----------------------------------------------------------------------------------------------------------------
// a: the SOURCE plane h x w, the output oh x ow
__global__ __launch_bounds__(kBlock) void pyr_up_kernel(PyrArgs a)
{
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break;
        const Tile tl = tile_of(a, u);
        const int ox = tl.x0 + 4 * lx;
        if (ox >= a.ow) continue;
        const size_t in_base = (size_t)tl.f * (size_t)a.h * (size_t)a.w, out_base = (size_t)tl.f * (size_t)a.oh * (size_t)a.ow;
        // the source columns sx - 1 .. sx + 2 under the output columns ox .. ox + 3, by the rule's ends:
        // s[-1] := s[min(1, w - 1)], s[w] := s[w - 1] (columns past that feed only pixels that do not exist)
        const int sx = ox >> 1;
        int cx[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = sx - 1 + k;
            cx[k] = c < 0 ? min(1, a.w - 1) : min(c, a.w - 1);
        }
        for (int blk = 0; blk < 2; blk++) {
            const int oy = tl.y0 + 2 * (ly + 8 * blk);
            if (oy >= a.oh) break;
            const int sy = oy >> 1;
            unsigned ev[3], od[3]; // per source row: the sums of the even output columns (ox, ox + 2) and of the odd ones
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int c = sy - 1 + j;
                const size_t row = in_base + (size_t)(c < 0 ? min(1, a.h - 1) : min(c, a.h - 1)) * (size_t)a.w;
                const unsigned s0 = load_px(a.src, 0, row + cx[0]), s1 = load_px(a.src, 0, row + cx[1]);
                const unsigned s2 = load_px(a.src, 0, row + cx[2]), s3 = load_px(a.src, 0, row + cx[3]);
                const unsigned p01 = s0 | (s1 << 16), p12 = s1 | (s2 << 16), p23 = s2 | (s3 << 16);
                ev[j] = p01 + 6u * p12 + p23; // (s0 + 6 s1 + s2, s1 + 6 s2 + s3)
                od[j] = 4u * (p12 + p23);     // (4 (s1 + s2), 4 (s2 + s3))
            }
            const int nv = a.ow - ox;
            for (int q = 0; q < 2; q++) {
                if (oy + q >= a.oh) break;
                const unsigned e = (q ? 4u * (ev[1] + ev[2]) : ev[0] + 6u * ev[1] + ev[2]) + 0x00200020u;
                const unsigned o = (q ? 4u * (od[1] + od[2]) : od[0] + 6u * od[1] + od[2]) + 0x00200020u;
                // e: pixels 0 and 2, o: pixels 1 and 3
                const unsigned pe = (e >> 6) & kEven, po = (o >> 6) & kEven;
                const unsigned lo = (pe & 0xFFu) | ((po & 0xFFu) << 16), hi = (pe >> 16) | (po & 0x00FF0000u);
                store_four(a.dst, out_base + (size_t)(oy + q) * (size_t)a.ow + (size_t)ox, nv, lo, hi);
            }
        }
    }
}

PyrArgs make_args(const void *src, bool src_s16, int n_frames, int h, int w, int oh, int ow, uint8_t *out, LaunchPlan *plan)
{
    *plan = plan_pyramid_tiles(n_frames, oh, ow);
    PyrArgs a;
    a.src = src, a.dst = out, a.h = h, a.w = w, a.oh = oh, a.ow = ow;
    a.n_units = plan->units, a.trips = (unsigned)plan->trips();
    a.tiles_x = (unsigned)((ow + kTW - 1) / kTW), a.tiles_y = (unsigned)((oh + kTH - 1) / kTH);
    a.src_s16 = src_s16;
    return a;
}

bool plane_ok(int n_frames, int h, int w)
{
    return n_frames >= 1 && n_frames <= 65535 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && (long long)h * w < (1ll << 31);
}

} // namespace

LaunchPlan plan_pyramid_tiles(int n_frames, int out_h, int out_w)
{
    const unsigned long long tiles = (((unsigned long long)out_w + kTW - 1) / kTW) * (((unsigned long long)out_h + kTH - 1) / kTH);
    return capped_plan(tiles * (unsigned long long)n_frames, 1, kGridCap);
}

int pyramid_auto_route()
{
    // DESIGN.md section 40 has the measurements this line follows
    return 2;
}

hipError_t launch_pyr_down(const void *src, bool src_s16, int n_frames, int h, int w, int route, uint8_t *out, hipStream_t stream)
{
    if (!src || !out || !plane_ok(n_frames, h, w) || route < 0 || route > 2) return hipErrorInvalidValue;
    LaunchPlan p;
    const PyrArgs a = make_args(src, src_s16, n_frames, h, w, (h + 1) / 2, (w + 1) / 2, out, &p);
    if ((route ? route : pyramid_auto_route()) == 1)
        hipLaunchKernelGGL(pyr_down_direct_kernel, dim3(p.grid), dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(pyr_down_tiled_kernel, dim3(p.grid), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pyr_up(const uint8_t *src, int n_frames, int h, int w, int oh, int ow, uint8_t *out, hipStream_t stream)
{
    if (!src || !out || !plane_ok(n_frames, h, w) || !plane_ok(n_frames, oh, ow) || (oh != 2 * h - 1 && oh != 2 * h) ||
        (ow != 2 * w - 1 && ow != 2 * w))
        return hipErrorInvalidValue;
    LaunchPlan p;
    const PyrArgs a = make_args(src, false, n_frames, h, w, oh, ow, out, &p);
    hipLaunchKernelGGL(pyr_up_kernel, dim3(p.grid), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace canny
