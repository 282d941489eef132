// canny_gray_morph.hip -- grey-level morphology and median filtering of u8 planes: erode, dilate, open, close, gradient, top
// hat and black hat with the binary morphology's flat elements of up to 31 x 31 offsets, the median of the full 3 x 3 or 5 x 5
// window, three outside-of-frame rules and iterations.  The rule is part of the interface (include/canny_hip.h, DESIGN.md
// section 39); tests/gray_morph_rule.py restates it in numpy, canny_gray_morph_host.cpp pixel by pixel in plain C++.  All
// integer minima, maxima and differences; every output byte has one writer; no atomics: the same bytes on every run.
//
//   One primitive step (an erosion, a dilation or a median) is one launch: a workgroup of 256 lanes per tile of 128 columns x
//   32 rows and trip of a capped grid; a lane owns four adjacent pixels (one 32-bit word) of four rows.  A step is "combine
//   over the offsets b of in(p + b)": min for the erosion, max for the dilation with the element reflected by the launcher,
//   so that the kernel knows one direction only.
//   stage     : the tile's bytes plus kh / 2 rows above and below and up to 16 columns left and right go to LDS as 32-bit
//               words of four pixels.  The outside-of-frame rule is put in HERE -- the step's constant (the neutral value or
//               the caller's) or the clamped coordinate -- and nowhere else: no lane tests a pixel afterwards.
//   bytes     : gfx950 has packed 16-bit min / max and no packed 8-bit ones.  A word of four pixels becomes two words of two
//               16-bit lanes (even = w & 0x00FF00FF, odd = (w >> 8) & 0x00FF00FF); pk_min / pk_max work on those.  A
//               horizontal offset is v_alignbyte over two neighbouring words, a vertical offset another staged row.
//   general   : per output word and per non-empty element row (wave-uniform scalars from the kernel arguments) every set
//               offset of the row's runs: two LDS words, one alignbyte, two packed combinations.
//   separable : a full rectangle: the horizontal run of kw by doubling (windows of 1, 2, 4, .. and once the rest) between two
//               LDS arrays, then the vertical run of kh the same way, a barrier a pass: about 2 (log2(k) + 1) passes.
//   median    : counting (per pixel the smallest window value with more than (k^2 - 1) / 2 values at or below it) or a
//               min / max selection network on the packed lanes (canny_gray_median.h: 19 exchanges for 3 x 3, 99 for 5 x 5).
//   last step : the saturating difference of GRADIENT, TOPHAT and BLACKHAT belongs to the last step's kernel, which reads the
//               other operand from global memory: max(a, b) - b on the 16-bit lanes never borrows.
//   store     : a whole word where the four columns are inside the frame and the address is 4-byte aligned, bytes otherwise.
#include "canny_gray_median.h"
#include "canny_kernels.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 128, kTH = 32;       // output tile: columns x rows
constexpr int kLaneRows = 4;             // rows of a lane; its columns are the four of one word
constexpr int kMaxExt = 31, kHalo = 15;  // CANNY_HIP_MORPH_MAX_EXTENT and its half
constexpr int kPad = 16;                 // staged columns left and right of the tile: the halo rounded up to whole words
constexpr int kSW = (kTW + 2 * kPad) / 4; // staged words of a row
constexpr int kSH = kTH + 2 * kHalo;     // staged rows at most
constexpr int kLds = kSH * kSW + 8;      // a pass reads up to 8 words past a row's end (into cells nobody needs)
constexpr unsigned kGridCap = 4096;
constexpr unsigned kEven = 0x00FF00FFu;

static_assert(kTW / 4 * (kTH / kLaneRows) == kBlock, "one lane per word of four rows of the tile");
static_assert(kPad >= kHalo && kPad % 4 == 0, "the halo fits into the staged pad, in whole words");

struct GrayArgs {
    const void *src, *other; // other: the operand of the last step's difference, or null
    uint8_t *dst;
    int h, w;
    unsigned long long n_units;
    unsigned trips, tiles_x, tiles_y;
    int kw, kh;
    unsigned rows[kMaxExt]; // as the kernel reads them: reflected for a dilation
    int replicate;          // the outside reads the clamped coordinate; otherwise `fill`
    unsigned fill;          // 0..255
    int combine;            // 0: out = r; 1: out = sat(r - other); 2: out = sat(other - r)
    int src_s16, other_s16; // a plane of shorts in [0, 255] (the context's smoothed plane) instead of bytes
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
template <bool MAX>
__device__ __forceinline__ unsigned comb(unsigned a, unsigned b)
{
    return MAX ? pk_max(a, b) : pk_min(a, b);
}
// the same on the four bytes of a word
template <bool MAX>
__device__ __forceinline__ unsigned comb4(unsigned a, unsigned b)
{
    return comb<MAX>(a & kEven, b & kEven) | (comb<MAX>((a >> 8) & kEven, (b >> 8) & kEven) << 8);
}
// the four bytes that start `shift` (0..3) bytes into lo, continued in hi
__device__ __forceinline__ unsigned bytes_at(unsigned lo, unsigned hi, int shift)
{
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)shift);
}

__device__ __forceinline__ unsigned load_px(const void *p, int s16, size_t i)
{
    return s16 ? (unsigned)static_cast<const uint16_t *>(p)[i] & 0xFFu : (unsigned)static_cast<const uint8_t *>(p)[i];
}

struct Tile {
    unsigned f;
    int x0, y0, th, sh, wlo, nw; // th output rows, sh staged rows, the staged words [wlo, wlo + nw) of a row
};

__device__ __forceinline__ Tile tile_of(const GrayArgs &a, unsigned long long u)
{
    const unsigned per_frame = a.tiles_x * a.tiles_y;
    const unsigned f = (unsigned)(u / per_frame), t = (unsigned)(u % per_frame);
    Tile tl;
    tl.f = f, tl.x0 = (int)(t % a.tiles_x) * kTW, tl.y0 = (int)(t / a.tiles_x) * kTH;
    tl.th = min(kTH, a.h - tl.y0), tl.sh = tl.th + a.kh - 1;
    const int ax = a.kw >> 1;
    tl.wlo = (kPad - ax) >> 2, tl.nw = ((kPad + kTW + ax + 3) >> 2) - tl.wlo;
    return tl;
}

// The staged window of the tile: row sy is frame row y0 - kh / 2 + sy, word k the columns x0 - kPad + 4 k .. + 3.  Every
// global read is inside frame f: the border rule answers for the rest.
__device__ __forceinline__ void stage(const GrayArgs &a, const Tile &tl, unsigned *s)
{
    const size_t fbase = (size_t)tl.f * (size_t)a.h * (size_t)a.w;
    const int ay = a.kh >> 1;
    const unsigned fill4 = a.fill * 0x01010101u;
    for (int i = threadIdx.x; i < tl.sh * tl.nw; i += kBlock) {
        const int sy = i / tl.nw, k = tl.wlo + (i - sy * tl.nw);
        int gy = tl.y0 - ay + sy;
        const int gx = tl.x0 - kPad + 4 * k;
        if (a.replicate) gy = min(max(gy, 0), a.h - 1);
        unsigned v = fill4;
        if (gy >= 0 && gy < a.h) {
            const size_t row = fbase + (size_t)gy * (size_t)a.w;
            const uint8_t *p8 = static_cast<const uint8_t *>(a.src) + row + gx;
            if (gx >= 0 && gx + 3 < a.w && !a.src_s16 && !((uintptr_t)p8 & 3)) {
                v = *reinterpret_cast<const unsigned *>(p8);
            } else {
                v = 0;
                for (int j = 0; j < 4; j++) {
                    int x = gx + j;
                    if (a.replicate) x = min(max(x, 0), a.w - 1);
                    const unsigned b = (x < 0 || x >= a.w) ? a.fill : load_px(a.src, a.src_s16, row + (size_t)x);
                    v |= b << (8 * j);
                }
            }
        }
        s[sy * kSW + k] = v;
    }
}

// The lane's word of row y, columns x .. x + 3 (e: pixels 0 and 2, o: pixels 1 and 3), with the last step's difference.
__device__ __forceinline__ void store_word(const GrayArgs &a, unsigned f, int y, int x, unsigned e, unsigned o)
{
    const size_t idx = ((size_t)f * (size_t)a.h + (size_t)y) * (size_t)a.w + (size_t)x;
    const int nv = min(4, a.w - x);
    if (a.combine) {
        unsigned q = 0;
        for (int j = 0; j < nv; j++) q |= load_px(a.other, a.other_s16, idx + j) << (8 * j);
        const unsigned qe = q & kEven, qo = (q >> 8) & kEven;
        if (a.combine == 1)
            e = pk_max(e, qe) - qe, o = pk_max(o, qo) - qo; // max(a, b) - b: no lane borrows from its neighbour
        else
            e = pk_max(qe, e) - e, o = pk_max(qo, o) - o;
    }
    const unsigned v = e | (o << 8);
    uint8_t *d = a.dst + idx;
    if (nv == 4 && !((uintptr_t)d & 3)) {
        *reinterpret_cast<unsigned *>(d) = v;
    } else {
        for (int j = 0; j < nv; j++) d[j] = (uint8_t)(v >> (8 * j));
    }
}

template <bool MAX>
__global__ __launch_bounds__(kBlock) void gray_general_kernel(GrayArgs a)
{
    __shared__ unsigned s_in[kLds];
    const int ax = a.kw >> 1;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const Tile tl = tile_of(a, u);
        __syncthreads(); // the last trip has read its LDS
        stage(a, tl, s_in);
        __syncthreads();
        const int x = tl.x0 + 4 * lx;
        if (x >= a.w) continue;
        for (int r = 0; r < kLaneRows; r++) {
            const int oy = ly * kLaneRows + r;
            if (oy >= tl.th) break;
            unsigned e = MAX ? 0u : kEven, o = e;
            for (int j = 0; j < a.kh; j++) {
                unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)a.rows[j]);
                const unsigned *p = s_in + (oy + j) * kSW;
                while (m) {
                    const int i = __builtin_ctz(m);
                    m &= m - 1;
                    const int col = kPad + 4 * lx + i - ax; // >= kPad - ax >= 1
                    const int k = col >> 2;
                    const unsigned v = bytes_at(p[k], p[k + 1], col & 3);
                    e = comb<MAX>(e, v & kEven), o = comb<MAX>(o, (v >> 8) & kEven);
                }
            }
            store_word(a, tl.f, tl.y0 + oy, x, e, o);
        }
    }
}

template <bool MAX>
__global__ __launch_bounds__(kBlock) void gray_separable_kernel(GrayArgs a)
{
    __shared__ unsigned s_a[kLds], s_b[kLds];
    const int ax = a.kw >> 1;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const Tile tl = tile_of(a, u);
        __syncthreads(); // the last trip has read its LDS
        stage(a, tl, s_a);
        __syncthreads();
        unsigned *from = s_a, *to = s_b;
        // R[c] = the combination of in[c .. c + kw - 1] along the row.  The cells an output needs, staged columns kPad - ax ..
        // kPad + kTW - 1 + ax, read nothing right of column kPad + kTW - 1 + ax < 4 kSW; what a pass reads beyond is junk
        // that ends in cells nobody needs.
        for (int n = 1; n < a.kw;) {
            const int s = 2 * n <= a.kw ? n : a.kw - n; // doubling, then once the rest
            const int q = s >> 2, sh = s & 3;
            for (int i = threadIdx.x; i < tl.sh * tl.nw; i += kBlock) {
                const int sy = i / tl.nw, c = sy * kSW + tl.wlo + (i - sy * tl.nw);
                to[c] = comb4<MAX>(from[c], bytes_at(from[c + q], from[c + q + 1], sh));
            }
            __syncthreads();
            unsigned *const tmp = from;
            from = to, to = tmp;
            n += s;
        }
        // V[sy] = the combination of R[sy .. sy + kh - 1] down the column; the rows below sh - kh are not read
        for (int n = 1; n < a.kh;) {
            const int s = 2 * n <= a.kh ? n : a.kh - n;
            for (int i = threadIdx.x; i < tl.sh * tl.nw; i += kBlock) {
                const int sy = i / tl.nw, c = sy * kSW + tl.wlo + (i - sy * tl.nw);
                to[c] = sy + s < tl.sh ? comb4<MAX>(from[c], from[c + s * kSW]) : from[c];
            }
            __syncthreads();
            unsigned *const tmp = from;
            from = to, to = tmp;
            n += s;
        }
        const int x = tl.x0 + 4 * lx;
        if (x >= a.w) continue;
        const int col = kPad + 4 * lx - ax, k = col >> 2; // the window of output column x starts ax to its left
        for (int r = 0; r < kLaneRows; r++) {
            const int oy = ly * kLaneRows + r;
            if (oy >= tl.th) break;
            const unsigned *p = from + oy * kSW;
            const unsigned v = bytes_at(p[k], p[k + 1], col & 3);
            store_word(a, tl.f, tl.y0 + oy, x, v & kEven, (v >> 8) & kEven);
        }
    }
}

#define CANNY_GRAY_EXCHANGE(i, j)                                                                                                \
    {                                                                                                                            \
        const unsigned lo_e = pk_min(e[i], e[j]), lo_o = pk_min(o[i], o[j]);                                                     \
        e[j] = pk_max(e[i], e[j]), o[j] = pk_max(o[i], o[j]);                                                                    \
        e[i] = lo_e, o[i] = lo_o;                                                                                                \
    }

// K: 3 or 5; NET: the selection network, otherwise the rank by counting
template <int K, bool NET>
__global__ __launch_bounds__(kBlock) void gray_median_kernel(GrayArgs a)
{
    __shared__ unsigned s_in[kLds];
    constexpr int A = K / 2, N = K * K, R = (N - 1) / 2;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const Tile tl = tile_of(a, u);
        __syncthreads(); // the last trip has read its LDS
        stage(a, tl, s_in);
        __syncthreads();
        const int x = tl.x0 + 4 * lx;
        if (x >= a.w) continue;
        for (int r = 0; r < kLaneRows; r++) {
            const int oy = ly * kLaneRows + r;
            if (oy >= tl.th) break;
            unsigned e[N], o[N]; // the window of the lane's four pixels: value t of pixels 0, 2 and of pixels 1, 3
#pragma unroll
            for (int j = 0; j < K; j++) {
                const unsigned *p = s_in + (oy + j) * kSW + kPad / 4 + lx;
                const unsigned l = p[-1], c = p[0], rr = p[1];
#pragma unroll
                for (int i = 0; i < K; i++) {
                    const int dx = i - A;
                    const unsigned v = dx < 0 ? bytes_at(l, c, 4 + dx) : (dx == 0 ? c : bytes_at(c, rr, dx));
                    e[j * K + i] = v & kEven, o[j * K + i] = (v >> 8) & kEven;
                }
            }
            unsigned me, mo;
            if constexpr (NET) {
                if constexpr (K == 3) {
                    CANNY_GRAY_MED9_NET(CANNY_GRAY_EXCHANGE)
                    me = e[CANNY_GRAY_MED9_OUT], mo = o[CANNY_GRAY_MED9_OUT];
                } else {
                    CANNY_GRAY_MED25_NET(CANNY_GRAY_EXCHANGE)
                    me = e[CANNY_GRAY_MED25_OUT], mo = o[CANNY_GRAY_MED25_OUT];
                }
            } else {
                // the smallest value with more than R window values at or below it is the R-th smallest (counted from 0)
                me = mo = 0;
                for (int px = 0; px < 4; px++) {
                    const int sh = (px & 2) ? 16 : 0;
                    unsigned v[N];
#pragma unroll
                    for (int t = 0; t < N; t++) v[t] = (((px & 1) ? o[t] : e[t]) >> sh) & 0xFFu;
                    unsigned best = 255u;
#pragma unroll
                    for (int t = 0; t < N; t++) {
                        int at_or_below = 0;
#pragma unroll
                        for (int q = 0; q < N; q++) at_or_below += v[q] <= v[t] ? 1 : 0;
                        if (at_or_below > R) best = min(best, v[t]);
                    }
                    if (px & 1)
                        mo |= best << sh;
                    else
                        me |= best << sh;
                }
            }
            store_word(a, tl.f, tl.y0 + oy, x, me, mo);
        }
    }
}
#undef CANNY_GRAY_EXCHANGE

bool full_rectangle(const unsigned *rows, int kw, int kh)
{
    for (int j = 0; j < kh; j++)
        if (rows[j] != (1u << kw) - 1u) return false;
    return true;
}

// What one primitive step reads and writes.  kind: 0 erode, 1 dilate, 2 median.
struct Step {
    const void *src;
    bool src_s16;
    uint8_t *dst;
    int kind;
    const void *other;
    bool other_s16;
    int combine;
};

hipError_t launch_step(const Step &s, int n_frames, int h, int w, const unsigned *rows, int kw, int kh, int border_mode,
                       int border_value, int route, hipStream_t stream)
{
    const LaunchPlan p = plan_gray_morph_tiles(n_frames, h, w);
    GrayArgs a;
    a.src = s.src, a.other = s.other, a.dst = s.dst, a.h = h, a.w = w;
    a.n_units = p.units, a.trips = (unsigned)p.trips();
    a.tiles_x = (unsigned)((w + kTW - 1) / kTW), a.tiles_y = (unsigned)((h + kTH - 1) / kTH);
    a.kw = kw, a.kh = kh;
    for (int j = 0; j < kMaxExt; j++) a.rows[j] = 0;
    for (int j = 0; j < kh; j++) {
        if (s.kind != 1) {
            a.rows[j] = rows[j];
        } else { // in(p - b): the element reflected through its centre
            unsigned m = 0;
            for (int i = 0; i < kw; i++) m |= ((rows[kh - 1 - j] >> i) & 1u) << (kw - 1 - i);
            a.rows[j] = m;
        }
    }
    a.replicate = border_mode == 1;
    a.fill = border_mode == 0 ? (s.kind == 1 ? 0u : 255u) : (unsigned)border_value; // NEUTRAL: a property of the step
    a.combine = s.combine, a.src_s16 = s.src_s16, a.other_s16 = s.other_s16;
    const int op_class = s.kind == 2 ? 7 : 0;
    const bool fast = (s.kind == 2 || full_rectangle(rows, kw, kh)) &&
                      (route == 2 || (route == 0 && gray_morph_auto_route(op_class, kw, kh) == 2));
    const dim3 grid(p.grid), block(kBlock);
    if (s.kind == 2) {
        if (kw == 3) {
            if (fast)
                hipLaunchKernelGGL((gray_median_kernel<3, true>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((gray_median_kernel<3, false>), grid, block, 0, stream, a);
        } else {
            if (fast)
                hipLaunchKernelGGL((gray_median_kernel<5, true>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((gray_median_kernel<5, false>), grid, block, 0, stream, a);
        }
    } else if (s.kind == 1) {
        if (fast)
            hipLaunchKernelGGL((gray_separable_kernel<true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((gray_general_kernel<true>), grid, block, 0, stream, a);
    } else {
        if (fast)
            hipLaunchKernelGGL((gray_separable_kernel<false>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((gray_general_kernel<false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace

LaunchPlan plan_gray_morph_tiles(int n_frames, int h, int w)
{
    const unsigned long long tiles = (((unsigned long long)w + kTW - 1) / kTW) * (((unsigned long long)h + kTH - 1) / kTH);
    return capped_plan(tiles * (unsigned long long)n_frames, 1, kGridCap);
}

int gray_morph_auto_route(int op, int kw, int kh)
{
    // DESIGN.md section 39 has the measurements this line follows (128 x 4K, ERODE): 3 x 3 general 1.43 ms against separable
    // 1.75; 5 x 5 2.39 against 2.28; 7 x 7 3.86 against 2.44; the networks 4.4 x and 9.9 x ahead of the counting rank
    if (op == 7) return 2;
    return kw * kh > 9 ? 2 : 1;
}

hipError_t launch_gray_morph(const void *src, bool src_s16, int n_frames, int h, int w, int op, const unsigned *rows, int kw,
                             int kh, int border_mode, int border_value, int iterations, int route, uint8_t *ws_a, uint8_t *ws_b,
                             uint8_t *out, hipStream_t stream)
{
    if (!src || !out || !rows || n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || op < 0 ||
        op > 7 || kw < 1 || kw > kMaxExt || kh < 1 || kh > kMaxExt || !(kw & 1) || !(kh & 1) || border_mode < 0 ||
        border_mode > 2 || (border_mode == 2 && (border_value < 0 || border_value > 255)) || iterations < 1 || iterations > 16 ||
        route < 0 || route > 2)
        return hipErrorInvalidValue;
    if (op == 7 && (kw != kh || (kw != 3 && kw != 5) || !full_rectangle(rows, kw, kh) || border_mode == 0))
        return hipErrorInvalidValue;
    const int n_steps = (op == 0 || op == 1 || op == 7 ? 1 : 2) * iterations;
    if ((n_steps > 1 && !ws_a) || (n_steps > 2 && !ws_b)) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    const auto step = [&](const Step &s) { return launch_step(s, n_frames, h, w, rows, kw, kh, border_mode, border_value, route, stream); };
    if (op == 4) {
        // GRADIENT = sat(DILATE - ERODE).  The erosions go src -> .. -> ws_a, alternating between ws_a and the caller's output
        // (every byte of which the last step writes anyway); the dilations alternate between ws_b and the output, the last
        // intermediate in ws_b, and the last step subtracts ws_a.
        const void *from = src;
        bool s16 = src_s16;
        for (int i = 1; i <= iterations && e == hipSuccess; i++) {
            uint8_t *to = ((iterations - i) & 1) ? out : ws_a;
            e = step(Step{from, s16, to, 0, nullptr, false, 0});
            from = to, s16 = false;
        }
        from = src, s16 = src_s16;
        for (int i = 1; i <= iterations && e == hipSuccess; i++) {
            const bool last = i == iterations;
            uint8_t *to = last ? out : (((iterations - 1 - i) & 1) ? out : ws_b);
            e = step(Step{from, s16, to, 1, last ? ws_a : nullptr, false, last ? 1 : 0});
            from = to, s16 = false;
        }
        return e;
    }
    // a chain src -> ws_a -> ws_b -> ws_a .. -> out; OPEN and TOPHAT erode first, CLOSE and BLACKHAT dilate first
    const bool first_dilate = op == 1 || op == 3 || op == 6;
    const void *from = src;
    bool s16 = src_s16;
    for (int i = 1; i <= n_steps && e == hipSuccess; i++) {
        const bool last = i == n_steps;
        const bool dilate = (op <= 1 || i <= iterations) ? first_dilate : !first_dilate;
        uint8_t *to = last ? out : ((i & 1) ? ws_a : ws_b);
        Step s{from, s16, to, op == 7 ? 2 : (dilate ? 1 : 0), nullptr, false, 0};
        if (last && op == 5) s.other = src, s.other_s16 = src_s16, s.combine = 2; // TOPHAT = sat(in - OPEN)
        if (last && op == 6) s.other = src, s.other_s16 = src_s16, s.combine = 1; // BLACKHAT = sat(CLOSE - in)
        e = step(s);
        from = to, s16 = false;
    }
    return e;
}

} // namespace canny
