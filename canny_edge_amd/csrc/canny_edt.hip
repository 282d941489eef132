// canny_edt.hip -- exact Euclidean distance transform of a finished edge map, per frame of a batch: for every pixel the
// squared distance to the nearest edge pixel (an integer), its correctly rounded root, and the index of that edge pixel
// (the smallest index among equally near ones).  scipy.ndimage.distance_transform_edt(~mask) / cv::distanceTransform(
// DIST_L2, DIST_MASK_PRECISE).  DESIGN.md section 15.
//
// The transform is separable (Meijster, Roerdink, Hesselink 2000; Felzenszwalb, Huttenlocher 2012):
//
//   rows     one wave per image row, one lane per 64-pixel word of the bit map.  The column of the last set pixel before a
//            word and of the first after it come from a wave scan (max / min over lanes; rows wider than 4096 pixels take
//            several rounds with a carry, the "first after" values of all words waiting in LDS).  Then the wave walks the
//            row word by word, lane = pixel: clz / ctz on the word masked to the bits at or below / at or above the lane
//            give the nearest set column on either side, a zero word takes the scan's values without looking at bits.
//            Stored is G(r,c), the COLUMN of the nearest set pixel of row r (u16, ties to the left, kEdtNoCol = none in
//            this row): 64 lanes x 2 bytes = one contiguous 128-byte line per store.
//   columns  dist2(x,c) = min over r of (x - r)^2 + (c - G(r,c))^2: the lower envelope of one parabola per row.  One lane
//            per column, a wave = 64 adjacent columns, so every row of G it reads is one 128-byte line.  A forward scan
//            builds the stack of (s, t) = (row of the parabola, first row it owns) with a strict pop (ties stay with the
//            smaller row); a backward scan walks the stack down and stores the planes, nearest = s * width + G(s,c).
//            A stack entry is s | t << 16 in a u32 plane [slot][column] -- the caller's dist2 plane when there is one
//            (slot q is read before row q is stored: t[q] >= q), a workspace otherwise -- plus G(s,c) in slot q of the
//            G plane itself (the forward scan has consumed rows 0 .. u when it writes slot q <= u).  The top of the
//            stack and the entry below it live in registers; a pop loads the next one down.
//
// No atomics; every output element is stored exactly once, by the lane that owns its column.  The launches depend on the
// shapes and on which planes were asked for, never on the data, and the work is O(height * width) per frame whatever
// the map holds (a row is pushed and popped at most once per column).
//
// Limits (checked by the callers): height * width < 2^31, height^2 + width^2 < 2^31 -- every intermediate below fits an
// int, rows and columns fit the u16 fields (both < 46341 < kEdtNoCol).
//
// Two sources, as canny_points.hip: the converged strong bit-plane (tile-major) or a caller's packed bit map (rows
// MSB-first, padded to bytes, any byte address; padding bits masked off).
#include "canny_kernels.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kEdtBlock = 256;                   // 4 waves
constexpr int kNoLeft = -100000, kNoRight = 200000; // "no set pixel on this side": farther than any real column, and
                                                    // c - kNoLeft <= kNoRight - c for every c < 46341 (both absent -> left)
constexpr unsigned kEdtNoCol = 0xFFFFu;

// ---- rows ------------------------------------------------------------------------------------------------------------
// cols: [n_frames][height][pitch] u16, pitch = 64 * tiles_x (the padding columns of a row are stored too, never read).
// A wave takes rows_per_wave consecutive rows: the strong plane keeps 8 rows of a word in one 64-byte line.
template <bool BITS>
__global__ __launch_bounds__(kEdtBlock) void edt_rows_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                             int rows_per_wave, uint16_t *__restrict__ cols)
{
    extern __shared__ int s_right[]; // [wave of the block][word of the row]: first set column after the word
    const int lane = threadIdx.x & 63;
    int *right = s_right + (threadIdx.x >> 6) * g.tiles_x;
    const size_t pitch = (size_t)g.tiles_x << 6;
    const size_t n_rows = (size_t)g.n_frames * g.height;
    const size_t n_groups = (n_rows + rows_per_wave - 1) / rows_per_wave;
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull); // bits 0 .. lane
    const uint64_t from = ~0ull << lane;                                // bits lane .. 63
    const int last_round = ((g.tiles_x - 1) >> 6) << 6;
    for (size_t grp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, stride = ((size_t)gridDim.x * blockDim.x) >> 6;
         grp < n_groups; grp += stride) {
        const size_t r_end = min(n_rows, (grp + 1) * rows_per_wave);
        for (size_t r = grp * rows_per_wave; r < r_end; r++) {
            const int f = (int)(r / (size_t)g.height), y = (int)(r - (size_t)f * g.height);
            // right to left: the first set column after each word
            int carry = kNoRight;
            for (int k0 = last_round; k0 >= 0; k0 -= 64) {
                const int k = k0 + lane;
                const uint64_t w = k < g.tiles_x ? row_word<BITS>(src, g, row_bytes, f, y, k) : 0ull;
                int incl = w ? (k << 6) + (int)__builtin_ctzll(w) : kNoRight;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_down(incl, d);
                    if (lane + d < 64) incl = min(incl, t);
                }
                int excl = __shfl_down(incl, 1);
                if (lane == 63) excl = kNoRight;
                if (k < g.tiles_x) right[k] = min(excl, carry);
                carry = min(carry, __shfl(incl, 0));
            }
            // left to right: the last set column before each word, then the row's pixels word by word
            int lcarry = kNoLeft;
            for (int k0 = 0; k0 < g.tiles_x; k0 += 64) {
                const int k = k0 + lane;
                const uint64_t w = k < g.tiles_x ? row_word<BITS>(src, g, row_bytes, f, y, k) : 0ull;
                int incl = w ? (k << 6) + 63 - (int)__builtin_clzll(w) : kNoLeft;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_up(incl, d);
                    if (lane >= d) incl = max(incl, t);
                }
                int before = __shfl_up(incl, 1);
                if (lane == 0) before = kNoLeft;
                before = max(before, lcarry);
                lcarry = max(lcarry, __shfl(incl, 63));
                const int after = k < g.tiles_x ? right[k] : kNoRight; // written by this lane in the loop above
                const int words = min(64, g.tiles_x - k0);
                uint16_t *out = cols + r * pitch + ((size_t)k0 << 6) + lane;
                for (int i = 0; i < words; i++) {
                    const uint64_t wi = __shfl(w, i); // wave-uniform
                    const int base = (k0 + i) << 6;
                    int cl = __shfl(before, i), cr = __shfl(after, i);
                    if (wi) {
                        const uint64_t lo = wi & upto, hi = wi & from;
                        if (lo) cl = base + 63 - (int)__builtin_clzll(lo);
                        if (hi) cr = base + (int)__builtin_ctzll(hi);
                    }
                    const int c = base + lane;
                    const int col = (c - cl <= cr - c) ? cl : cr; // ties to the left
                    out[(size_t)i << 6] = (uint16_t)(col < 0 ? kEdtNoCol : (unsigned)col);
                }
            }
        }
    }
}

// ---- columns ---------------------------------------------------------------------------------------------------------
struct Parabola {
    int s, t, col; // row, first row it owns, G(s, c)
};

// cols and stack are read AND written (see the head of the file); stack may be dist2.
__global__ __launch_bounds__(kEdtBlock) void edt_columns_kernel(uint16_t *cols, HystGeom g, uint32_t *stack,
                                                                size_t stack_pitch, int *dist2, float *dist, int *nearest)
{
    const int lane = threadIdx.x & 63;
    const int H = g.height, W = g.width;
    const size_t pitch = (size_t)g.tiles_x << 6;
    const size_t frame_px = (size_t)H * W;
    const size_t n_items = (size_t)g.n_frames * g.tiles_x;
    for (size_t item = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6,
                stride = ((size_t)gridDim.x * blockDim.x) >> 6;
         item < n_items; item += stride) {
        const int f = (int)(item / (size_t)g.tiles_x);
        const int c = ((int)(item - (size_t)f * g.tiles_x) << 6) + lane;
        if (c >= W) continue; // nothing below is wave-wide
        uint16_t *gc = cols + (size_t)f * H * pitch + c;        // G(r, c) at gc[r * pitch]; slot q's column at gc[q * pitch]
        uint32_t *st = stack + (size_t)f * H * stack_pitch + c; // slot q at st[q * stack_pitch]
        int q = -1;                                             // index of the top of the stack
        Parabola top{0, 0, 0}, below{0, 0, 0};                  // slots q and q - 1 (valid while q >= 0 / q >= 1)
        auto pop = [&]() {
            q--;
            top = below;
            if (q >= 1) {
                const uint32_t e = st[(size_t)(q - 1) * stack_pitch];
                below.s = (int)(e & 0xFFFFu), below.t = (int)(e >> 16), below.col = (int)gc[(size_t)(q - 1) * pitch];
            }
        };
        // forward: the lower envelope.  A row without a set pixel has no parabola (the same rows for every column).
        for (int u0 = 0; u0 < H; u0 += 8) {
            unsigned gv[8];
#pragma unroll
            for (int j = 0; j < 8; j++) gv[j] = u0 + j < H ? (unsigned)gc[(size_t)(u0 + j) * pitch] : kEdtNoCol;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (gv[j] == kEdtNoCol) continue;
                const int u = u0 + j, gu = (int)gv[j];
                const int hu = c - gu, fu = hu * hu;
                while (q >= 0) { // strict: where both are equally near, the smaller row keeps the pixel
                    const int ht = c - top.col, dt = top.t - top.s, du = top.t - u;
                    if (dt * dt + ht * ht <= du * du + fu) break;
                    pop();
                }
                int t = 0;
                if (q >= 0) {
                    // first row at which u is strictly nearer than top.s; the numerator is >= 0 (top.s is no farther
                    // than u at row top.t >= 0), so the unsigned division is the floor
                    const int ht = c - top.col;
                    const unsigned num = (unsigned)(((u * u - top.s * top.s) + fu) - ht * ht);
                    t = (int)(num / (unsigned)(2 * (u - top.s))) + 1;
                    if (t >= H) continue; // u owns no row of this column
                }
                q++;
                below = top;
                top = Parabola{u, t, gu};
                // slot q <= u (at most one push per row): in dist2 no row has been stored yet; in the G plane rows
                // 0 .. u of this column are consumed (u0 .. u0 + 7 sit in gv), and only this lane touches the column
                st[(size_t)q * stack_pitch] = (uint32_t)u | ((uint32_t)t << 16);
                gc[(size_t)q * pitch] = (uint16_t)gu;
            }
        }
        // backward: every row takes the parabola that owns it
        int *d2_out = dist2 ? dist2 + (size_t)f * frame_px + c : nullptr;
        float *d_out = dist ? dist + (size_t)f * frame_px + c : nullptr;
        int *n_out = nearest ? nearest + (size_t)f * frame_px + c : nullptr;
        for (int x = H - 1; x >= 0; x--) {
            int d2 = 0x7FFFFFFF, at = -1;
            float d = __builtin_inff();
            if (q >= 0) {
                while (x < top.t) pop();
                const int dx = x - top.s, hx = c - top.col;
                d2 = dx * dx + hx * hx;
                at = top.s * W + top.col;
                if (d_out) d = (float)sqrt((double)d2);
            }
            const size_t o = (size_t)x * W;
            // when the stack lives in dist2 this overwrites slot x.  The owner q of row x has t[q] <= x, and t grows by
            // at least 1 per slot from t[0] = 0, so q <= x: slot q is in `top`, slot q - 1 in `below`, and every slot a
            // later pop loads lies below x
            if (d2_out) d2_out[o] = d2;
            if (d_out) d_out[o] = d;
            if (n_out) n_out[o] = at;
        }
    }
}

} // namespace

LaunchPlan plan_edt_rows(const HystGeom &g)
{
    const unsigned long long n_rows = (unsigned long long)g.n_frames * g.height;
    const int rows_per_wave = n_rows >= (1u << 16) ? 8 : 1; // enough waves for the chip either way
    return capped_plan((n_rows + rows_per_wave - 1) / rows_per_wave, kEdtBlock / 64, 1u << 16, rows_per_wave);
}
LaunchPlan plan_edt_columns(const HystGeom &g)
{
    return capped_plan((unsigned long long)g.n_frames * g.tiles_x, kEdtBlock / 64, 1u << 16);
}

hipError_t launch_edt_rows(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, uint16_t *cols,
                           hipStream_t stream)
{
    const LaunchPlan plan = plan_edt_rows(g);
    const int rows_per_wave = plan.aux;
    const unsigned grid = plan.grid;
    const size_t lds = (size_t)(kEdtBlock / 64) * g.tiles_x * sizeof(int); // < 12 KiB at the widest row
    const int row_bytes = (g.width + 7) / 8;
    if (bits)
        hipLaunchKernelGGL(edt_rows_kernel<true>, dim3(grid), dim3(kEdtBlock), lds, stream, (const void *)bits, g,
                           row_bytes, rows_per_wave, cols);
    else
        hipLaunchKernelGGL(edt_rows_kernel<false>, dim3(grid), dim3(kEdtBlock), lds, stream, (const void *)strong, g,
                           row_bytes, rows_per_wave, cols);
    return hipGetLastError();
}

hipError_t launch_edt_columns(const HystGeom &g, uint16_t *cols, uint32_t *stack, int *dist2, float *dist, int *nearest,
                              hipStream_t stream)
{
    const size_t stack_pitch = stack ? edt_pitch(g) : (size_t)g.width;
    if (!stack) stack = reinterpret_cast<uint32_t *>(dist2);
    hipLaunchKernelGGL(edt_columns_kernel, dim3(plan_edt_columns(g).grid), dim3(kEdtBlock), 0, stream,
                       cols, g, stack, stack_pitch, dist2, dist, nearest);
    return hipGetLastError();
}

} // namespace canny
