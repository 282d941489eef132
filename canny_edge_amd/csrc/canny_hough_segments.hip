// canny_hough_segments.hip -- Hough line SEGMENTS: the runs of edge pixels along each detected line, per frame of a batch
// (the deterministic counterpart of cv::HoughLinesP).  The rule is part of the interface (include/canny_hip.h, DESIGN.md
// section 16); tests/hough_segments_rule.py restates it in numpy on the full plane.
//
// A line is an accumulator cell (n, r).  Its support are the set pixels whose vote for angle n is r -- vote_r of
// canny_kernels.h, the vote kernels' own function, so these are exactly the pixels that voted for the cell.  Along the
// line's major axis (x if |sin| >= |cos|) position t is `on` if any pixel of the support has that coordinate; on positions
// at most max_gap off positions apart form a run; a run at least min_length long is a segment.
//
// The walk: lanes take 64 consecutive t.  For its t a lane solves the line for the minor coordinate in float and tests the
// few integers around that estimate with the EXACT vote (the estimate only bounds the search: what counts is vote == r),
// then looks the survivors up in the bit map.  `on` becomes a 64-bit ballot; the previous on position of a lane is a mask
// and a count-leading-zeros on it; run starts are a second ballot that a scalar loop walks, reading the prefix sums of the
// counts with v_readlane.  The open run (start, its minor coordinate, support so far) and the last on position cross the
// chunks in wave-uniform registers.
//
//   non-exclusive: one wave per (frame, line); count pass -> scan over the frame's lines -> emit pass, as the point lists do,
//                  so that the records land in (line, start) order without any atomic.
//   exclusive:     one workgroup per frame takes the lines in list order on a private copy of the map: all 16 waves probe
//                  1024 positions at a time into LDS, wave 0 splits the runs (it carries the running output offset, so one
//                  pass suffices) and marks kept positions in an LDS bit set; then all waves clear the support of the kept
//                  positions from the copy with workgroup-scope 32-bit atomic ANDs.  Workgroup barriers separate the
//                  phases and the lines; the copy is read with workgroup-scope atomic loads.  Workgroup scope suffices
//                  because no 32-bit word of the copy is shared between frames: the strong plane's frames are whole
//                  64-bit words, and packed bytes are copied to a stride of their own per frame.  The kernel is handed
//                  the copy alone (the source pointers of its SegSrc are null): it cannot write the plane or d_bits.
#include "canny_line_support.h"

#include <algorithm>
#include <cmath>

namespace canny {

namespace {

constexpr int kSegBlock = 256;   // non-exclusive: four waves, four lines
constexpr int kExclBlock = 1024; // exclusive: 16 waves share one frame

// SegSrc, bit_of, pixel_set_src, SegLine, seg_line and seg_window live in canny_line_support.h: the line fits walk the same
// support.
template <bool BITS, bool EXCL>
__device__ __forceinline__ bool pixel_set(const SegSrc &src, const HystGeom &g, int row_bytes, int f, int y, int x)
{
    if constexpr (EXCL) {
        size_t word;
        unsigned mask;
        bit_of<BITS>(g, row_bytes, src.work_frame_words, f, y, x, &word, &mask);
        return (__hip_atomic_load(&src.work[word], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & mask) != 0;
    } else {
        return pixel_set_src<BITS>(src, g, row_bytes, f, y, x);
    }
}

// The support of the line at major position t: how many pixels (return value) and the smallest minor coordinate (*lo).
// CLEAR: instead, every pixel of the support is cleared from the working copy.
template <bool BITS, bool EXCL, bool CLEAR>
__device__ __forceinline__ int probe(const SegSrc &src, const HystGeom &g, int row_bytes, int f, const SegLine &ln,
                                     float halfwin, int t, int *lo)
{
    int cnt = 0, ma, mb;
    *lo = 0;
    if (!seg_window(ln, halfwin, t, &ma, &mb)) return 0; // off the frame (or no estimate at all)
    for (int m = ma; m <= mb; m++) {
        const int x = ln.major_x ? t : m, y = ln.major_x ? m : t;
        if (vote_r(x, y, ln.c, ln.s, ln.half) != ln.r) continue;
        if (!pixel_set<BITS, EXCL>(src, g, row_bytes, f, y, x)) continue;
        if constexpr (CLEAR) {
            size_t word;
            unsigned mask;
            bit_of<BITS>(g, row_bytes, src.work_frame_words, f, y, x, &word, &mask);
            __hip_atomic_fetch_and(&src.work[word], ~mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            if (!cnt) *lo = m; // ascending m: the first is the smallest
        }
        cnt++;
    }
    return cnt;
}

// What crosses the 64-position chunks of a line; every member is wave-uniform.
struct RunState {
    int ta = -1, lo_ta = 0; // the open run's first position and its minor coordinate; -1 = no run yet
    int last = -1, lo_last = 0; // the last on position so far and its minor coordinate
    int support = 0;        // the open run's support in the chunks before this one
};

__device__ __forceinline__ int lane_value(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// One chunk: lane i holds cnt / lo of position t0 + i (cnt 0 past the line's end).  close(ta, lo_ta, tb, lo_tb, support) is
// called, in ascending order and by the whole wave, for every run that ends in front of a run start of this chunk.
template <class Close>
__device__ __forceinline__ void split_chunk(RunState &st, int t0, int cnt, int lo, int max_gap, Close &&close)
{
    const uint64_t on = __ballot(cnt > 0);
    if (!on) return;
    const int lane = threadIdx.x & 63;
    int incl = cnt; // inclusive prefix of the counts
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    const uint64_t below = on & ((1ull << lane) - 1ull);
    const int prev = below ? t0 + 63 - (int)__builtin_clzll(below) : st.last;
    uint64_t starts = __ballot(cnt > 0 && (prev < 0 || t0 + lane - prev - 1 > max_gap));
    int base = 0; // prefix in front of the open run's first position of this chunk
    while (starts) {
        const int j = (int)__builtin_ctzll(starts);
        starts &= starts - 1ull;
        const uint64_t bj = on & ((1ull << j) - 1ull);
        const int pj = bj ? 63 - (int)__builtin_clzll(bj) : -1; // the on position in front of the start, if in this chunk
        const int upto = pj >= 0 ? lane_value(incl, pj) : 0;
        if (st.ta >= 0)
            close(st.ta, st.lo_ta, pj >= 0 ? t0 + pj : st.last, pj >= 0 ? lane_value(lo, pj) : st.lo_last,
                  st.support + upto - base);
        st.ta = t0 + j;
        st.lo_ta = lane_value(lo, j);
        st.support = 0;
        base = upto;
    }
    const int pl = 63 - (int)__builtin_clzll(on);
    st.support += lane_value(incl, 63) - base;
    st.last = t0 + pl;
    st.lo_last = lane_value(lo, pl);
}

// record j of a frame: lanes 0..5 store one int each
__device__ __forceinline__ void store_record(int *__restrict__ rec, const SegLine &ln, int ta, int lo_ta, int tb, int lo_tb,
                                             int k, int support)
{
    const int lane = threadIdx.x & 63;
    if (lane >= kSegRecord) return;
    const int x0 = ln.major_x ? ta : lo_ta, y0 = ln.major_x ? lo_ta : ta;
    const int x1 = ln.major_x ? tb : lo_tb, y1 = ln.major_x ? lo_tb : tb;
    rec[lane] = lane == 0 ? x0 : lane == 1 ? y0 : lane == 2 ? x1 : lane == 3 ? y1 : lane == 4 ? k : support;
}

// grid (ceil(lines_max / 4), n_frames); one wave per line.  !EMIT: nseg[slot] = the line's segments.  EMIT: the records.
template <bool BITS, bool EMIT>
__global__ __launch_bounds__(kSegBlock) void seg_walk_kernel(SegSrc src, HystGeom g, int row_bytes,
                                                             const float *__restrict__ tab, SegGeom sg,
                                                             const unsigned *__restrict__ bases,
                                                             const int *__restrict__ line_counts, int *__restrict__ nseg,
                                                             const int *__restrict__ line_off, int *__restrict__ segments)
{
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * (kSegBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= min(sg.lines_max, line_counts[f])) return;
    const size_t slot = (size_t)f * sg.lines_max + k;
    SegLine ln;
    int found = 0;
    if (seg_line(bases[slot], tab, sg.numangle, sg.numrho, g, ln)) {
        const int off = EMIT ? line_off[slot] : 0;
        int *out = segments + (size_t)f * sg.segments_max * kSegRecord;
        auto close = [&](int ta, int lo_ta, int tb, int lo_tb, int support) {
            if (tb - ta < sg.min_length) return;
            if constexpr (EMIT) {
                const int j = off + found;
                if (j < sg.segments_max) store_record(out + (size_t)j * kSegRecord, ln, ta, lo_ta, tb, lo_tb, k, support);
            }
            found++;
        };
        RunState st;
        for (int t0 = 0; t0 < ln.L; t0 += 64) {
            const int t = t0 + lane;
            int lo = 0;
            const int cnt = t < ln.L ? probe<BITS, false, false>(src, g, row_bytes, f, ln, sg.halfwin, t, &lo) : 0;
            split_chunk(st, t0, cnt, lo, sg.max_gap, close);
        }
        if (st.ta >= 0) close(st.ta, st.lo_ta, st.last, st.lo_last, st.support);
    }
    if constexpr (!EMIT)
        if (lane == 0) nseg[slot] = found;
}

// one workgroup per frame: line_off = exclusive prefix of nseg over the frame's lines, seg_counts[f] = their sum
__global__ __launch_bounds__(kSegBlock) void seg_scan_kernel(const int *__restrict__ line_counts, int lines_max,
                                                             const int *__restrict__ nseg, int *__restrict__ line_off,
                                                             int *__restrict__ seg_counts)
{
    __shared__ int s_wave[kSegBlock / 64];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = min(lines_max, line_counts[f]);
    int carry = 0;
    for (int k0 = 0; k0 < K; k0 += kSegBlock) {
        const int k = k0 + (int)threadIdx.x;
        const int v = k < K ? nseg[(size_t)f * lines_max + k] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(incl, d);
            if (lane >= d) incl += u;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < kSegBlock / 64; w++) {
            const int u = s_wave[w];
            if (w < wave) before += u;
            sum += u;
        }
        __syncthreads();
        if (k < K) line_off[(size_t)f * lines_max + k] = carry + before + incl - v;
        carry += sum;
    }
    if (threadIdx.x == 0) seg_counts[f] = carry;
}

// grid (n_frames); dynamic LDS: 1024 counts | 1024 minor coordinates | one bit per major position
template <bool BITS>
__global__ __launch_bounds__(kExclBlock) void seg_exclusive_kernel(SegSrc src, HystGeom g, int row_bytes,
                                                                   const float *__restrict__ tab, SegGeom sg,
                                                                   const unsigned *__restrict__ bases,
                                                                   const int *__restrict__ line_counts,
                                                                   int *__restrict__ segments, int *__restrict__ seg_counts)
{
    extern __shared__ int s_mem[];
    __shared__ int s_kept_any;
    int *s_cnt = s_mem, *s_lo = s_mem + kExclBlock;
    unsigned *s_keep = (unsigned *)(s_mem + 2 * kExclBlock);
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const bool wave0 = tid < 64;
    const int K = min(sg.lines_max, line_counts[f]);
    int *out = segments + (size_t)f * sg.segments_max * kSegRecord;
    int total = 0; // wave 0: segments of the frame so far
    for (int k = 0; k < K; k++) {
        SegLine ln;
        // the same for every thread
        if (!seg_line(bases[(size_t)f * sg.lines_max + k], tab, sg.numangle, sg.numrho, g, ln)) continue;
        for (int i = tid; i < (ln.L + 31) / 32; i += kExclBlock) s_keep[i] = 0u;
        if (tid == 0) s_kept_any = 0;
        auto close = [&](int ta, int lo_ta, int tb, int lo_tb, int support) { // wave 0
            if (tb - ta < sg.min_length) return;
            if (total < sg.segments_max) store_record(out + (size_t)total * kSegRecord, ln, ta, lo_ta, tb, lo_tb, k, support);
            total++;
            for (int w = (ta >> 5) + lane; w <= (tb >> 5); w += 64) {
                const int first = max(ta - (w << 5), 0), last = min(tb - (w << 5), 31);
                s_keep[w] |= (0xffffffffu >> (31 - last)) & (0xffffffffu << first);
            }
            s_kept_any = 1;
        };
        RunState st;
        for (int p0 = 0; p0 < ln.L; p0 += kExclBlock) {
            const int t = p0 + tid;
            int lo = 0;
            s_cnt[tid] = t < ln.L ? probe<BITS, true, false>(src, g, row_bytes, f, ln, sg.halfwin, t, &lo) : 0;
            s_lo[tid] = lo;
            __syncthreads();
            if (wave0)
                for (int c = 0; c < kExclBlock && p0 + c < ln.L; c += 64)
                    split_chunk(st, p0 + c, s_cnt[c + lane], s_lo[c + lane], sg.max_gap, close);
            __syncthreads();
        }
        if (wave0 && st.ta >= 0) close(st.ta, st.lo_ta, st.last, st.lo_last, st.support);
        __syncthreads();
        if (s_kept_any) {
            for (int t = tid; t < ln.L; t += kExclBlock) {
                int lo;
                if (s_keep[t >> 5] >> (t & 31) & 1u) (void)probe<BITS, true, true>(src, g, row_bytes, f, ln, sg.halfwin, t, &lo);
            }
        }
        __syncthreads(); // the next line sees the cleared copy
    }
    if (tid == 0) seg_counts[f] = total;
}

SegSrc make_src(const uint64_t *strong, const uint8_t *bits, uint32_t *work, size_t work_frame_words)
{
    return SegSrc{reinterpret_cast<const uint32_t *>(strong), bits, work, work_frame_words};
}

template <bool EMIT>
hipError_t launch_walk(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg, const float *tab,
                       const unsigned *bases, const int *line_counts, int *nseg, const int *line_off, int *segments,
                       hipStream_t stream)
{
    const dim3 grid((sg.lines_max + kSegBlock / 64 - 1) / (kSegBlock / 64), g.n_frames);
    const SegSrc src = make_src(strong, bits, nullptr, 0);
    if (bits)
        hipLaunchKernelGGL((seg_walk_kernel<true, EMIT>), grid, dim3(kSegBlock), 0, stream, src, g, (g.width + 7) / 8, tab,
                           sg, bases, line_counts, nseg, line_off, segments);
    else
        hipLaunchKernelGGL((seg_walk_kernel<false, EMIT>), grid, dim3(kSegBlock), 0, stream, src, g, (g.width + 7) / 8, tab,
                           sg, bases, line_counts, nseg, line_off, segments);
    return hipGetLastError();
}

} // namespace

// For one t the minor coordinates with vote == r lie within 0.7072 * rho of the real solution of the line (the vote moves
// by |c_minor| >= 1 / (rho * sqrt 2) per pixel and must stay within 1/2 of r); + 2 for the ends, + the float error of the
// vote's three operations and of the estimate, which scales with the magnitude of the products, (width + height) / rho.
float hough_segments_halfwin(int height, int width, float rho)
{
    const float top = ((float)width + (float)height) / rho + 1.0f;
    const float ulp = std::nextafter(top, INFINITY) - top;
    return 0.7072f * rho + 2.0f + 16.0f * rho * ulp;
}

hipError_t launch_hough_segments_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg,
                                       const float *tab, const unsigned *bases, const int *line_counts, int *nseg,
                                       int *line_off, int *seg_counts, hipStream_t stream)
{
    hipError_t e = launch_walk<false>(strong, bits, g, sg, tab, bases, line_counts, nseg, nullptr, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seg_scan_kernel, dim3(g.n_frames), dim3(kSegBlock), 0, stream, line_counts, sg.lines_max, nseg,
                       line_off, seg_counts);
    return hipGetLastError();
}

hipError_t launch_hough_segments_emit(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg,
                                      const float *tab, const unsigned *bases, const int *line_counts, const int *line_off,
                                      int *segments, hipStream_t stream)
{
    return launch_walk<true>(strong, bits, g, sg, tab, bases, line_counts, nullptr, line_off, segments, stream);
}

hipError_t launch_hough_segments_exclusive(uint32_t *work, bool work_is_bits, const HystGeom &g, const SegGeom &sg,
                                           const float *tab, const unsigned *bases, const int *line_counts, int *segments,
                                           int *seg_counts, hipStream_t stream)
{
    const int axis = std::max(g.height, g.width);
    if (axis > kSegExclusiveMaxAxis) return hipErrorInvalidValue;
    const size_t lds = (2 * (size_t)kExclBlock + ((size_t)axis + 31) / 32) * sizeof(int);
    const SegSrc src = make_src(nullptr, nullptr, work, hough_segments_work_stride(g) / sizeof(uint32_t));
    auto launch = [&](auto kernel) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, dim3(g.n_frames), dim3(kExclBlock), lds, stream, src, g, (g.width + 7) / 8, tab, sg,
                           bases, line_counts, segments, seg_counts);
        return hipGetLastError();
    };
    return work_is_bits ? launch(seg_exclusive_kernel<true>) : launch(seg_exclusive_kernel<false>);
}

} // namespace canny
