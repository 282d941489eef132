// canny_morph.hip -- binary morphology on packed bit maps: erode, dilate, open, close, gradient, top hat and black hat with
// elements of up to 31 x 31 offsets, an outside-of-frame rule and iterations.  The rule is part of the interface
// (include/canny_hip.h); tests/morph_rule.py restates it in numpy, canny_morph_host.cpp pixel by pixel in
// plain C++.  All bit operations; every output byte has one writer; the only atomic is the integer sum behind counts[f]: the
// same bytes on every run.
//
//   One primitive step (an erosion or a dilation) is one launch: a workgroup of 256 lanes per tile of 8 words x 64 rows (512 x
//   64 pixels) and trip of a capped grid.  A step is "combine over the offsets b of in(p + b)": AND for the erosion, OR for the
//   dilation with the element reflected by the launcher, so that the kernel knows one direction only.
//   stage     : the tile's words plus kh / 2 rows above and below and one word left and right go to LDS as LSB-first 64-bit
//               words (bit i = column 64 k + i).  The outside-of-frame value is put in HERE -- rows outside the frame, words
//               left and right of the frame, the columns >= w of the last word -- and nowhere else: no lane tests a pixel.
//   run       : a run of L set bits of an element row, starting at offset a, is the combination of the 128-bit window that
//               starts at column 64 k + a with itself shifted by 1, 2, 4, .. (doubling) and once by the rest: O(log L) shifts.
//   general   : per output word and per non-empty element row the three staged words of the row y + dy, the runs of the row's
//               mask (wave-uniform scalars from the kernel arguments), combined into the accumulator.
//   separable : a full rectangle: the horizontal run of every staged row into a second LDS array, then the vertical run by
//               doubling between the two arrays with a barrier a step: about 2 log2(31) combinations for 31 x 31.
//   last step : the combination with another map (GRADIENT, TOPHAT, BLACKHAT), the clearing of the pad bits and the per-frame
//               counts belong to the kernel of the last step.  A workgroup's trips are consecutive tiles, so a lane sums the
//               set bits of a frame over its trips and a wave adds to counts[f] once or twice, not once per tile.
#include "canny_bit_words.h" // flip_bits, morph_load, funnel
#include "canny_kernels.h"

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 8, kTH = 64;         // output tile: words (of 64 columns) x rows
constexpr int kMaxExt = 31, kHalo = 15;  // CANNY_HIP_MORPH_MAX_EXTENT and its half
constexpr int kSW = kTW + 2;             // staged words of a row: one to the left, one to the right
constexpr int kSH = kTH + 2 * kHalo;     // staged rows at most
constexpr unsigned kGridCap = 4096;

struct MorphArgs {
    const void *src, *other; // other: the map of the last step's combination, or null
    uint8_t *dst;
    unsigned long long *counts;
    HystGeom g; // tiles_x = the words of a row
    int rb;     // bytes of a packed row
    unsigned long long n_units;
    unsigned trips, tiles_x, tiles_y; // tiles of this kernel, not of g
    int kw, kh;
    unsigned rows[kMaxExt]; // as the kernel reads them: reflected for a dilation
    unsigned fill;          // what the outside reads as: 0 or 1
    int combine;            // 0: out = r; 1: out = r & ~other; 2: out = other & ~r
    int src_plane, other_plane; // the strong bit-plane of geometry g instead of a packed map
    int vec_src, vec_other, vec_dst; // packed map whose rows are whole, 8-byte aligned words
};

template <bool OR>
__device__ __forceinline__ uint64_t comb(uint64_t a, uint64_t b)
{
    return OR ? a | b : a & b;
}

// The combination of in(x + d) over d = d0 .. d0 + len - 1 for the 64 columns x of word k, by doubling on the 128-bit window
// (lo, hi) that starts at column 64 k + d0.  Bit 64 + i of the window is needed for i <= len - 2 <= 29 only, and the window
// holds true columns up to 64 + 63 - d0 >= 112: the word right of r is never missed.  d0, len: wave-uniform.
template <bool OR>
__device__ __forceinline__ uint64_t run(uint64_t l, uint64_t c, uint64_t r, int d0, int len)
{
    uint64_t lo = funnel(l, c, r, d0), hi = funnel(c, r, 0, d0);
    int n = 1;
    while (2 * n <= len) {
        const uint64_t tl = (lo >> n) | (hi << (64 - n)), th = hi >> n;
        lo = comb<OR>(lo, tl), hi = comb<OR>(hi, th);
        n *= 2;
    }
    if (n < len) {
        const int s = len - n;
        lo = comb<OR>(lo, (lo >> s) | (hi << (64 - s)));
    }
    return lo;
}

template <bool OR, bool SEP>
__global__ __launch_bounds__(kBlock) void morph_step_kernel(MorphArgs a)
{
    __shared__ uint64_t s_in[kSH * kSW];
    __shared__ uint64_t s_h[SEP ? kSH * kTW : 1];
    const int ax = a.kw >> 1, ay = a.kh >> 1;
    const uint64_t fill = a.fill ? ~0ull : 0ull;
    const unsigned per_frame = a.tiles_x * a.tiles_y;
    unsigned acc = 0, cur = 0; // this lane's set bits of frame `cur`, not yet added to counts[cur]
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const unsigned f = (unsigned)(u / per_frame), t = (unsigned)(u % per_frame);
        const int k0 = (int)(t % a.tiles_x) * kTW, y0 = (int)(t / a.tiles_x) * kTH;
        const int th = min(kTH, a.g.height - y0), sh = th + a.kh - 1;
        __syncthreads(); // the last trip has read its LDS
        for (int i = threadIdx.x; i < sh * kSW; i += kBlock) {
            const int sy = i / kSW, sx = i - sy * kSW;
            const bool unread = ax == 0 && (sx == 0 || sx == kSW - 1); // no horizontal offset: the halo words are not formed
            s_in[i] = unread ? 0ull
                             : morph_load(a.src, a.src_plane, a.vec_src, a.g, a.rb, (int)f, y0 - ay + sy, k0 - 1 + sx, fill);
        }
        __syncthreads();
        const uint64_t *res = nullptr; // SEP: where the vertical run ended
        if constexpr (SEP) {
            for (int i = threadIdx.x; i < sh * kTW; i += kBlock) {
                const int sy = i / kTW, ox = i - sy * kTW;
                const uint64_t *p = s_in + sy * kSW + ox;
                s_h[i] = run<OR>(p[0], p[1], p[2], -ax, a.kw);
            }
            __syncthreads();
            uint64_t *from = s_h, *to = s_in; // s_in is free from here on: kSH * kTW words fit in it
            int n = 1;
            while (n < a.kh) {
                const int s = 2 * n <= a.kh ? n : a.kh - n; // doubling, then once the rest
                for (int i = threadIdx.x; i < sh * kTW; i += kBlock) {
                    const int j = i + s * kTW;
                    to[i] = j < sh * kTW ? comb<OR>(from[i], from[j]) : from[i]; // the rows below sh - kh are not read
                }
                __syncthreads();
                uint64_t *const tmp = from;
                from = to, to = tmp;
                n += s;
            }
            res = from;
        }
        if (a.counts && f != cur) { // the same on every lane
            for (int o = 32; o; o >>= 1) acc += (unsigned)__shfl_xor((int)acc, o);
            if ((threadIdx.x & 63) == 0 && trip) atomicAdd(a.counts + cur, (unsigned long long)acc); // also a sum of 0:
            cur = f, acc = 0;                                                                         // no cost from content
        }
        for (int i = threadIdx.x; i < th * kTW; i += kBlock) {
            const int oy = i / kTW, ox = i - oy * kTW;
            const int y = y0 + oy, k = k0 + ox;
            if (k >= a.g.tiles_x) continue;
            uint64_t v;
            if constexpr (SEP) {
                v = res[i];
            } else {
                v = OR ? 0ull : ~0ull;
                for (int j = 0; j < a.kh; j++) {
                    unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)a.rows[j]);
                    if (!m) continue;
                    const uint64_t *p = s_in + (oy + j) * kSW + ox;
                    const uint64_t l = p[0], c = p[1], r = p[2];
                    while (m) {
                        const int first = __builtin_ctz(m);
                        const unsigned rest = ~(m >> first);
                        const int len = rest ? __builtin_ctz(rest) : 32;
                        v = comb<OR>(v, run<OR>(l, c, r, first - ax, len));
                        m &= len >= 32 - first ? 0u : ~0u << (first + len);
                    }
                }
            }
            if (a.combine) {
                const uint64_t o = morph_load(a.other, a.other_plane, a.vec_other, a.g, a.rb, (int)f, y, k, 0ull);
                v = a.combine == 1 ? v & ~o : o & ~v;
            }
            const int left = a.g.width - (k << 6);
            if (left < 64) v &= (1ull << left) - 1ull; // pad bits are written 0
            acc += (unsigned)__popcll(v);
            uint8_t *row = a.dst + ((size_t)f * a.g.height + y) * (size_t)a.rb + (size_t)k * 8;
            const uint64_t raw = flip_bits(v);
            if (a.vec_dst) {
                *reinterpret_cast<uint64_t *>(row) = raw;
            } else {
                const int nb = min(8, a.rb - k * 8);
                for (int j = 0; j < nb; j++) row[j] = (uint8_t)(raw >> (8 * j));
            }
        }
    }
    if (a.counts) {
        for (int o = 32; o; o >>= 1) acc += (unsigned)__shfl_xor((int)acc, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(a.counts + cur, (unsigned long long)acc);
    }
}

bool full_rectangle(const unsigned *rows, int kw, int kh)
{
    for (int j = 0; j < kh; j++)
        if (rows[j] != (1u << kw) - 1u) return false;
    return true;
}

bool vec_map(const void *p, int rb) { return !(rb & 7) && !((uintptr_t)p & 7); }

// What one primitive step reads and writes.
struct Step {
    const void *src;
    bool src_plane;
    uint8_t *dst;
    bool dilate;
    const void *other;
    bool other_plane;
    int combine;
    unsigned long long *counts;
};

hipError_t launch_step(const Step &s, const HystGeom &g, const unsigned *rows, int kw, int kh, int border, int route,
                       hipStream_t stream)
{
    const LaunchPlan p = plan_morph_tiles(g.n_frames, g.height, g.width);
    MorphArgs a;
    a.src = s.src, a.other = s.other, a.dst = s.dst, a.counts = s.counts, a.g = g, a.rb = (g.width + 7) / 8;
    a.n_units = p.units, a.trips = (unsigned)p.trips();
    a.tiles_x = (unsigned)((g.tiles_x + kTW - 1) / kTW), a.tiles_y = (unsigned)((g.height + kTH - 1) / kTH);
    a.kw = kw, a.kh = kh;
    for (int j = 0; j < kMaxExt; j++) a.rows[j] = 0;
    for (int j = 0; j < kh; j++) {
        if (!s.dilate) {
            a.rows[j] = rows[j];
        } else { // in(p - b): the element reflected through its centre
            unsigned m = 0;
            for (int i = 0; i < kw; i++) m |= ((rows[kh - 1 - j] >> i) & 1u) << (kw - 1 - i);
            a.rows[j] = m;
        }
    }
    a.fill = border == 2 ? (s.dilate ? 0u : 1u) : (unsigned)border; // NEUTRAL: a property of the step
    a.combine = s.combine, a.src_plane = s.src_plane, a.other_plane = s.other_plane;
    a.vec_src = !s.src_plane && vec_map(s.src, a.rb), a.vec_other = !s.other_plane && vec_map(s.other, a.rb);
    a.vec_dst = vec_map(s.dst, a.rb);
    const bool sep = full_rectangle(rows, kw, kh) && (route == 2 || (route == 0 && morph_auto_route(kw, kh) == 2));
    const dim3 grid(p.grid), block(kBlock);
    if (s.dilate) {
        if (sep)
            hipLaunchKernelGGL((morph_step_kernel<true, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((morph_step_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (sep)
            hipLaunchKernelGGL((morph_step_kernel<false, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((morph_step_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace

LaunchPlan plan_morph_tiles(int n_frames, int h, int w)
{
    const unsigned long long words = ((unsigned long long)w + 63) / 64;
    const unsigned long long tiles = ((words + kTW - 1) / kTW) * (((unsigned long long)h + kTH - 1) / kTH);
    return capped_plan(tiles * (unsigned long long)n_frames, 1, kGridCap);
}

int morph_auto_route(int kw, int kh)
{
    // separable is the faster route at 3 x 3, 7 x 7, 15 x 15 and 31 x 31 (ERODE and OPEN, both densities);
    // a single offset has no run to share and keeps the route without the second LDS array and its barrier
    return kw * kh > 1 ? 2 : 1;
}

hipError_t launch_morph(const void *src, bool src_plane, int n_frames, int h, int w, int op, const unsigned *rows, int kw,
                        int kh, int border, int iterations, int route, uint8_t *ws_a, uint8_t *ws_b, uint8_t *out,
                        unsigned long long *counts, hipStream_t stream)
{
    if (!src || !out || !rows || n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || op < 0 ||
        op > 6 || kw < 1 || kw > kMaxExt || kh < 1 || kh > kMaxExt || !(kw & 1) || !(kh & 1) || border < 0 || border > 2 ||
        iterations < 1 || iterations > 16 || route < 0 || route > 2 || ((uintptr_t)counts & 7))
        return hipErrorInvalidValue;
    const int n_steps = (op == 0 || op == 1 ? 1 : 2) * iterations;
    if ((n_steps > 1 && !ws_a) || (n_steps > 2 && !ws_b)) return hipErrorInvalidValue;
    if (counts) {
        const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_frames * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
    }
    const HystGeom g = make_hyst_geom(h, w, n_frames);
    hipError_t e = hipSuccess;
    if (op == 4) {
        // GRADIENT = DILATE & ~ERODE.  The erosions go src -> .. -> ws_a, alternating between ws_a and the caller's output
        // (every byte of which the last step writes anyway); the dilations alternate between ws_b and the output, the last
        // intermediate in ws_b, and the last step combines with ws_a.
        const void *from = src;
        bool plane = src_plane;
        for (int i = 1; i <= iterations && e == hipSuccess; i++) {
            uint8_t *to = ((iterations - i) & 1) ? out : ws_a;
            e = launch_step(Step{from, plane, to, false, nullptr, false, 0, nullptr}, g, rows, kw, kh, border, route, stream);
            from = to, plane = false;
        }
        from = src, plane = src_plane;
        for (int i = 1; i <= iterations && e == hipSuccess; i++) {
            const bool last = i == iterations;
            uint8_t *to = last ? out : (((iterations - 1 - i) & 1) ? out : ws_b);
            e = launch_step(Step{from, plane, to, true, last ? ws_a : nullptr, false, last ? 1 : 0, last ? counts : nullptr}, g,
                            rows, kw, kh, border, route, stream);
            from = to, plane = false;
        }
        return e;
    }
    // a chain src -> ws_a -> ws_b -> ws_a .. -> out; OPEN and TOPHAT erode first, CLOSE and BLACKHAT dilate first
    const bool first_dilate = op == 1 || op == 3 || op == 6;
    const void *from = src;
    bool plane = src_plane;
    for (int i = 1; i <= n_steps && e == hipSuccess; i++) {
        const bool last = i == n_steps;
        const bool dilate = (op <= 1 || i <= iterations) ? first_dilate : !first_dilate;
        uint8_t *to = last ? out : ((i & 1) ? ws_a : ws_b);
        Step s{from, plane, to, dilate, nullptr, false, 0, last ? counts : nullptr};
        if (last && op == 5) s.other = src, s.other_plane = src_plane, s.combine = 2; // TOPHAT = in & ~OPEN
        if (last && op == 6) s.other = src, s.other_plane = src_plane, s.combine = 1; // BLACKHAT = CLOSE & ~in
        e = launch_step(s, g, rows, kw, kh, border, route, stream);
        from = to, plane = false;
    }
    return e;
}

} // namespace canny
