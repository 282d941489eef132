// canny_kernels.h -- launchers for the gfx950 Canny kernels (internal; the public boundary is
// include/canny_hip.h).  All launchers are asynchronous on `stream` and return the launch status.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace canny {

constexpr int kMaxCenter = 64;                 // Gaussian half-window (window <= 129)
constexpr int kMaxWindow = 2 * kMaxCenter + 1;
constexpr int kTile = 64;                      // hysteresis bit-plane tile: 64 rows x 64 columns

// Gaussian taps exactly as the reference computes them on the host (src/utils.cpp:77-95); passed
// to kernels by value so they live in scalar registers / the kernarg segment.
struct GaussTaps {
    int center;
    float tap[kMaxWindow];
};

// Order in which the waves of a marching launch take the (segment, strip) cells of a frame: the frame's BORDER cells
// first (top and bottom segments, then the first and last strip of the segments in between), the interior cells after
// them.  Border cells run the border instantiations, which cost 1.1-1.7 x an interior cell; waves are dealt to SIMD
// slots in index order, so with the plain row-major order the last waves of a launch -- the bottom segment of the last
// frame -- were its most expensive ones and the chip waited for them with most slots empty.  Frames stay contiguous
// (and so do the interior cells of a frame, which share halo rows and columns in L2).  Bijective on [0, n_segs*n_strips).
struct MarchCell {
    int seg, strip;
};
__host__ __device__ inline MarchCell march_cell_of(int k, int n_segs, int n_strips)
{
    MarchCell c;
#ifdef CANNY_MARCH_ROW_MAJOR // A/B builds only: the plain order
    n_segs = 0;
#endif
    if (n_segs < 3 || n_strips < 3) { // every cell is a border cell
        c.seg = k / n_strips;
        c.strip = k % n_strips;
        return c;
    }
    const int sides = 2 * (n_segs - 2);
    if (k < n_strips) {
        c.seg = 0;
        c.strip = k;
    } else if (k < 2 * n_strips) {
        c.seg = n_segs - 1;
        c.strip = k - n_strips;
    } else if (k < 2 * n_strips + sides) {
        const int kk = k - 2 * n_strips;
        c.seg = 1 + (kk >> 1);
        c.strip = (kk & 1) ? n_strips - 1 : 0;
    } else {
        const int kk = k - 2 * n_strips - sides;
        c.seg = 1 + kk / (n_strips - 2);
        c.strip = 1 + kk % (n_strips - 2);
    }
    return c;
}

// Geometry of the hysteresis bit-planes: per frame tiles_y x tiles_x tiles, each 64 words (one
// 64-bit word = 64 consecutive pixels of one row), stored tile-major so that one wave reads a
// whole tile with one coalesced 512-byte load.
struct HystGeom {
    int height, width, n_frames;
    int tiles_x, tiles_y;
    __host__ __device__ size_t words() const { return (size_t)n_frames * tiles_x * tiles_y * kTile; }
    __host__ __device__ int tiles() const { return n_frames * tiles_x * tiles_y; }
};
inline HystGeom make_hyst_geom(int height, int width, int n_frames)
{
    HystGeom g;
    g.height = height;
    g.width = width;
    g.n_frames = n_frames;
    g.tiles_x = (width + kTile - 1) / kTile;
    g.tiles_y = (height + kTile - 1) / kTile;
    return g;
}

// ---- Gaussian (src/utils.cpp:26-68) ---------------------------------------------------------
// General two-pass path: any window up to kMaxWindow; tmp holds n_frames*H*W floats.
hipError_t launch_gaussian_generic(const uint8_t *img, float *tmp, int16_t *out, int height, int width,
                                   int n_frames, const GaussTaps &taps, hipStream_t stream);
// Wave-marching path for center <= 8 (window <= 17), row and column pass in one kernel: the symmetric-tap
// kernel (products shared between the +a / -a taps, column sums in registers) or, for asymmetric taps, the
// LDS-ring kernel (canny_gaussian_march.hip).
bool gaussian_march_supported(int center, int height, int width);
hipError_t launch_gaussian_march(const uint8_t *img, int16_t *out, int height, int width, int n_frames,
                                 const GaussTaps &taps, hipStream_t stream);

// The same kernel storing the smoothed plane as BYTES ((short)(sum/count) lies in [0,255], src/utils.cpp:62):
// half the store traffic, for the u8 form of the fused Sobel+NMS kernel.  Needs bit-symmetric taps and the default
// march variant.
bool gaussian_march_u8_supported(const GaussTaps &taps);
hipError_t launch_gaussian_march_u8(const uint8_t *img, uint8_t *out, int height, int width, int n_frames,
                                    const GaussTaps &taps, hipStream_t stream);

// (S, c) bit-pattern pairs for which the interior waves divide by the full-window weight S with one
// fma(a, c, a); returns the number of entries.  gaussian_set_fma_div(false) disables the shortcut
// process-wide (A/B measurements only).
int gaussian_fma_div_table(const unsigned (**table)[2]);
void gaussian_set_fma_div(bool on);
// A/B: 0 = symmetric-tap kernel (shared products, register accumulators) with the row-pass products looked up
// in an LDS table (default), 1 = LDS-ring kernel, 2 = symmetric-tap kernel that multiplies.
void gaussian_set_march_variant(int v);
void gaussian_set_seg_target(int rows); // A/B: approximate rows per wave segment, 0 = automatic

// ---- colour frames -> gray (what the reference's caller does with cvtColor, src/main.cpp:114) ----------------
// gray = (k0*c0 + k1*c1 + k2*c2 + rnd) >> shift for the first three bytes c0..c2 of an interleaved pixel (a fourth,
// alpha, is ignored).  The host orders the weights by the layout (BGR: k0 = wb, RGB: k0 = wr), so rules and channel
// orders are kernel arguments, not instantiations.  Every weight is < 2^16 and the sum < 2^24: 24-bit multiplies
// are exact.
struct GrayRule {
    uint32_t k0, k1, k2, rnd, shift;
};

// The ONE conversion of the library: four interleaved pixels of CH (3 or 4) bytes, i.e. CH dwords, -> the packed
// dword of their four gray bytes (pixel 0 in byte 0).  Both the standalone kernel and the fused Gaussian call it.
template <int CH>
__device__ __forceinline__ uint32_t gray4(const uint32_t *w, const GrayRule &r)
{
    static_assert(CH == 3 || CH == 4, "interleaved 3- or 4-byte pixels");
    uint32_t out = 0u;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = CH * p + k; // byte i of the 4*CH
            c[k] = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        }
        const uint32_t g = __umul24(c[0], r.k0) + __umul24(c[1], r.k1) + __umul24(c[2], r.k2) + r.rnd;
        out |= (g >> r.shift) << (8 * p);
    }
    return out;
}

// Standalone conversion of n_px interleaved pixels (the batch as one flat array; any source alignment) into
// n_px gray bytes.
hipError_t launch_to_gray(const uint8_t *src, int ch, const GrayRule &rule, uint8_t *gray, size_t n_px,
                          hipStream_t stream);

// The marching Gaussian (symmetric taps, systolic row pass with the product table, u8 output) reading interleaved
// CH-byte pixels and converting them as it loads its rows.  Windows listed by gaussian_march_color_supported only.
bool gaussian_march_color_supported(const GaussTaps &taps, int width, int ch);
hipError_t launch_gaussian_march_u8_color(const uint8_t *src, int ch, const GrayRule &rule, uint8_t *out, int height,
                                          int width, int n_frames, const GaussTaps &taps, hipStream_t stream);

// ---- Sobel / NMS (src/utils.cpp:106-308) ----------------------------------------------------
hipError_t launch_xy_gradient(const int16_t *img, int16_t *gx, int16_t *gy, int height, int width, int n_frames,
                              hipStream_t stream);
hipError_t launch_sobel(const int16_t *img, int16_t *mag, int16_t *angle, int height, int width, int n_frames,
                        hipStream_t stream);
hipError_t launch_nms(const int16_t *mag, const int16_t *angle, int16_t *out, int height, int width, int n_frames,
                      hipStream_t stream);
// Fused Sobel+NMS, LDS-tiled.  domain8 = smoothed plane known to lie in [0,255] (float sqrt + 24-bit
// products); otherwise the general path (double sqrt, 64-bit products).
hipError_t launch_sobel_nms(const int16_t *smoothed, int16_t *out, int height, int width, int n_frames,
                            bool domain8, hipStream_t stream);
// Fused Sobel+NMS, wave-marching and LDS-free (canny_sobel_nms_march.hip); smoothed must lie in [0,255].
bool sobel_nms_march_supported(int height, int width);
void sobel_nms_set_px_variant(int v); // A/B: 0 = 8 pixels per lane, 1 = 4 pixels per lane (more resident waves)
void sobel_nms_set_arith_variant(int v); // 0 = automatic (f32 for the fused classify kernel, packed-i16 for s16 -> s16), 1 = packed-i16, 2 = f32
// A/B (fused kernel): 0 = plane bytes staged in LDS for 8 rows and written as 8-byte words, 1 = direct byte stores
void sobel_nms_set_plane_store_variant(int v);
// An event pair attached to one kernel dispatch (hipExtLaunchKernel): that kernel's begin and end timestamps.
// Unlike hipEventRecord before and after the launch it puts no barrier packets into the stream (those cost
// ~30 us of stream time per pair).  Both null: plain launch.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
hipError_t launch_sobel_nms_march(const int16_t *smoothed, int16_t *out, int height, int width, int n_frames,
                                  hipStream_t stream, int tune_seg = 0, const LaunchEvents &ev = {});

// Fused Sobel+NMS+classify: the same marching kernel, but instead of the s16 suppressed magnitudes it
// writes the two hysteresis bit-planes that launch_hyst_classify would derive from them (in-image bytes
// only: pair it with launch_hyst_prepare(..., zero_pad = true)) and the provisional edge map `edges`
// (strong pixels -> edge_value, everything else 0) that launch_hyst_propagate(..., edges, edge_value) completes.
// Needs width % 8 == 0 and min_val >= 1.
// pairs != nullptr: per-frame thresholds (clamp_thresholds applied to each, edge_value must then be 255); a separate
// instantiation, so the kernels of the fixed-threshold call compile exactly as without it.
bool sobel_nms_classify_supported(int height, int width, int min_val);
hipError_t launch_sobel_nms_classify_march(const int16_t *smoothed, int16_t *edges, uint64_t *strong, uint64_t *conn,
                                           const HystGeom &g, int min_val, int max_val, int edge_value,
                                           hipStream_t stream, int tune_seg = 0, const LaunchEvents &ev = {},
                                           const int *pairs = nullptr);

// The two marching kernels reading the smoothed plane as BYTES (8 pixels per lane, LDS-staged planes only).
bool sobel_nms_u8_input_supported();
hipError_t launch_sobel_nms_march_u8in(const uint8_t *smoothed, int16_t *out, int height, int width, int n_frames,
                                       hipStream_t stream, int tune_seg = 0, const LaunchEvents &ev = {});
hipError_t launch_sobel_nms_classify_march_u8in(const uint8_t *smoothed, int16_t *edges, uint64_t *strong,
                                                uint64_t *conn, const HystGeom &g, int min_val, int max_val,
                                                int edge_value, hipStream_t stream, int tune_seg = 0,
                                                const LaunchEvents &ev = {}, const int *pairs = nullptr);

// ---- per-frame hysteresis thresholds (canny_hip_*_thresholds, canny_hip_*_auto) ----------
// A pair array holds (min_val, max_val) of frame f at [2f], [2f+1].  Every consumer clamps a pair into the domain
// 1 <= min_val <= max_val <= 255 first: there the edge map is the reference's for that pair, promoted pixels are
// always 255 and the scan-order-dependent case (hysteresis_order_dependent) cannot occur.
__host__ __device__ inline void clamp_thresholds(int &lo, int &hi)
{
    lo = lo < 1 ? 1 : (lo > 255 ? 255 : lo);
    hi = hi < lo ? lo : (hi > 255 ? 255 : hi);
}

constexpr int kAutoMedian = 1, kAutoQuantile = 2; // CANNY_HIP_AUTO_*
constexpr int kHistBins = 257;                     // per-frame histograms: values 0..255, and 256 = "256 or more"

// Q(q) = min { b : h[0] + ... + h[b] >= max(1, ceil(q * N)) } on a cumulative histogram cum(b) (N = cum(256)),
// in IEEE double like the host restatement.  257 when no bin reaches the count (N = 0).
template <class Cum>
__host__ __device__ inline int hist_quantile(const Cum &cum, double q)
{
    const double t = ceil(q * (double)cum(kHistBins - 1));
    const unsigned long long need = t < 1.0 ? 1ull : (unsigned long long)t;
    int a = 0, b = kHistBins; // smallest index in [a, b) whose count reaches `need`, b if none
    while (a < b) {
        const int m = (a + b) >> 1;
        if (cum(m) >= need)
            b = m;
        else
            a = m + 1;
    }
    return a;
}

// THE selection rule (host export canny_hip_auto_thresholds_from_histogram and the device select kernel):
//   median:   m = Q(0.5), (floor(low * m), floor(high * m))   on the smoothed plane's histogram
//   quantile: (Q(low), Q(high))                                on the histogram of min(magnitude, 256)
// then clamp_thresholds.  Parameters are validated by the caller (0 <= low <= high finite; quantile 0 < low <= high <= 1).
template <class Cum>
__host__ __device__ inline void auto_thresholds(const Cum &cum, int rule, double low, double high, int &lo, int &hi)
{
    if (rule == kAutoMedian) {
        const double m = (double)hist_quantile(cum, 0.5);
        // (products above 256 clamp to 255 anyway; capping first keeps the conversion to int defined)
        lo = (int)floor(fmin(low * m, 256.0));
        hi = (int)floor(fmin(high * m, 256.0));
    } else {
        lo = hist_quantile(cum, low);
        hi = hist_quantile(cum, high);
    }
    clamp_thresholds(lo, hi);
}

// Histograms of n_frames planes into hist[n_frames][kHistBins] (u32, must be zero beforehand; integer atomics, so
// the counts are exact whatever the order).  The plane is the smoothed one, bytes (in_u8) or shorts in [0,255].
//   intensity: bin = value
//   gradient:  bin = min(magnitude, 256) of the reference's Sobel (sobelOperator, its border rule) on that plane
hipError_t launch_hist_intensity(const void *plane, bool in_u8, uint32_t *hist, int height, int width, int n_frames,
                                 hipStream_t stream);
hipError_t launch_hist_gradient(const void *plane, bool in_u8, uint32_t *hist, int height, int width, int n_frames,
                                hipStream_t stream);
// One wave per frame: the rule above on hist[f] -> pairs[2f], pairs[2f+1].
hipError_t launch_thr_select(const uint32_t *hist, int n_frames, int rule, double low, double high, int *pairs,
                             hipStream_t stream);

// ---- Hysteresis (src/utils.cpp:322-427) -----------------------------------------------------
// pairs != nullptr: per-frame thresholds (clamp_thresholds applied to each; min_val / max_val are then ignored)
hipError_t launch_hyst_classify(const int16_t *cand, uint64_t *strong, uint64_t *conn, const HystGeom &g, int min_val,
                                int max_val, unsigned *domain_flag, hipStream_t stream, const int *pairs = nullptr);
// One propagation sweep (`iter` = 0,1,2,...).  sched holds hyst_sched_words(g) words (tile stamps, two batch-wide
// work queues with three counters, two per-frame work queues with four counter words per frame) and, like the
// single word last_change, must be zero before sweep 0.
inline size_t hyst_sched_words(const HystGeom &g) { return 5 * (size_t)g.tiles() + 4 + 4 * (size_t)g.n_frames; }
// First launch of a hysteresis call: zeroes sched (hyst_sched_words(g) words) and flags[0..1] (last_change,
// domain) and, if zero_pad, the plane bits outside the image (tile padding; needed when the planes are filled
// by launch_sobel_nms_classify_march, which writes in-image bytes only; requires width % 8 == 0).
// n_lanes > 1: the frames are propagated as n_lanes independent ranges (each with its own scheduling words, laid
// out back to back -- 3 * tiles + 4 * n_lanes words in all -- and its own pair of flags: 2 * n_lanes words).
hipError_t launch_hyst_prepare(uint64_t *strong, uint64_t *conn, const HystGeom &g, bool zero_pad, unsigned *sched,
                               unsigned *flags, hipStream_t stream, int n_lanes = 1);
// edges != nullptr: an edge map that already holds the initially strong pixels; each sweep writes edge_value
// into the pixels it promotes, so the map is final when propagation has converged (no finalize pass).
// frame_queues: the route that ends in launch_hyst_tail (frames of at most 4096 tiles).  The tiles a sweep schedules go
// into their FRAME's queue, and a sweep >= 1 walks those queues, a few workgroups per frame: the appends of a batch meet
// on one counter word per frame instead of one per batch.  All sweeps of a call use the same setting.
hipError_t launch_hyst_propagate(uint64_t *strong, const uint64_t *conn, unsigned *sched, unsigned *last_change,
                                 int iter, const HystGeom &g, hipStream_t stream, int16_t *edges = nullptr,
                                 int edge_value = 0, bool frame_queues = false);
// Every sweep from first_iter on, to convergence, in ONE launch: one workgroup per frame walks that frame's queue
// with a workgroup barrier between sweeps (frames are independent; see hyst_tail_kernel).  The sweeps before it
// must have been launched with frame_queues = true.  No host round trip: the propagation is complete when the
// stream has passed this kernel.
hipError_t launch_hyst_tail(uint64_t *strong, const uint64_t *conn, unsigned *sched, unsigned *last_change,
                            int first_iter, const HystGeom &g, hipStream_t stream, int16_t *edges = nullptr,
                            int edge_value = 0);
// s16 edge map (0 / 255) -> u8, n pixels.
hipError_t launch_edges_to_u8(const int16_t *edges, uint8_t *out, size_t n, hipStream_t stream);
// s16 edge map -> packed bit map (1 = pixel != 0), rows MSB-first and padded to bytes: [n][height][(width + 7) / 8]
hipError_t launch_edges_to_bits(const int16_t *edges, uint8_t *bits, int height, int width, int n_frames,
                                hipStream_t stream);
// Copies flags[0..1] (last_change, domain) to host_flags_dev[0..1] and then stores seq to host_flags_dev[2]
// (system-scope release); host_flags_dev is the device view of pinned, mapped host memory.
hipError_t launch_hyst_publish(const unsigned *flags, unsigned *host_flags_dev, unsigned seq, hipStream_t stream);
hipError_t launch_hyst_finalize(int16_t *cand, const uint64_t *strong, const HystGeom &g, int edge_value,
                                hipStream_t stream);
void hyst_set_finalize_mode(int mode); // A/B: 0 = row-major kernel (default), 1 = 8-row patch kernel
// findEdgePixels (single frame): seed = {start}, connectable = cand >= min_val && !visited.
hipError_t launch_fep_classify(const int16_t *cand, const uint8_t *visited, uint64_t *strong, uint64_t *conn,
                               const HystGeom &g, int start, int min_val, hipStream_t stream);
hipError_t launch_fep_finalize(int16_t *cand, uint8_t *visited, const uint64_t *strong, const HystGeom &g, int start,
                               int min_val, hipStream_t stream);

// ---- Edge point lists (canny_points.hip) -------------------------------
// Word of the bit-planes that holds columns 64*wx .. 64*wx + 63 of row y of frame f (word_index() of canny_kernels.hip).
__host__ __device__ inline size_t hyst_word_index(const HystGeom &g, int f, int y, int wx)
{
    return ((((size_t)f * g.tiles_y + (y >> 6)) * g.tiles_x + wx) << 6) + (y & 63);
}
// The source is the strong plane of geometry g, or -- bits != nullptr -- a packed bit map (rows MSB-first, padded to
// bytes, any byte address; padding bits ignored).
#ifdef __HIPCC__
// Columns 64*k .. 64*k + 63 of row y of frame f of either source (BITS: the packed map, row_bytes = (width + 7) / 8), bit i
// = column 64*k + i, columns >= width cleared.  0 <= y < height, 0 <= k < tiles_x.
template <bool BITS>
__device__ __forceinline__ uint64_t row_word(const void *__restrict__ src, const HystGeom &g, int row_bytes, int f,
                                             int y, int k)
{
    const int left = g.width - (k << 6); // > 0
    const uint64_t mask = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    if constexpr (!BITS) {
        return static_cast<const uint64_t *>(src)[hyst_word_index(g, f, y, k)] & mask;
    } else {
        const uint8_t *row = static_cast<const uint8_t *>(src) + ((size_t)f * g.height + y) * (size_t)row_bytes +
                             (size_t)k * 8;
        const int nb = min(8, row_bytes - k * 8);
        uint64_t w = 0;
        for (int j = 0; j < nb; j++) w |= (uint64_t)(__brev((unsigned)row[j]) >> 24) << (8 * j); // MSB-first -> LSB-first
        return w & mask;
    }
}
#endif
// count: row_counts[f * height + y] = set pixels of that row.
hipError_t launch_points_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, uint32_t *row_counts,
                               hipStream_t stream);
// scan: rows (in place) -> set pixels of the frame before the row; frame_totals[f] = the frame's count;
// offsets[0 .. n_frames] = exclusive prefix of the totals.
hipError_t launch_points_scan(uint32_t *rows, unsigned long long *frame_totals, unsigned long long *offsets, int height,
                              int n_frames, hipStream_t stream);
// scatter: points[offsets[f] + row_offsets[f * height + y] + k] = y * width + (k-th set column of the row), for every
// position below capacity; nothing is stored at or beyond points + capacity.
hipError_t launch_points_scatter(const uint64_t *strong, const uint8_t *bits, const HystGeom &g,
                                 const uint32_t *row_offsets, const unsigned long long *offsets, uint32_t *points,
                                 unsigned long long capacity, hipStream_t stream);

// ---- Hough lines (canny_hough.hip) -------------------------------------
struct HoughGeom {
    int numangle, numrho;
    float rho, theta, min_theta;
};
constexpr int kHoughMaxLines = 4096;          // CANNY_HIP_HOUGH_MAX_LINES: the sort's keys of one frame fit in LDS
constexpr int kHoughLdsMax = 160 * 1024;      // what one workgroup may declare on gfx950
inline size_t hough_accum_bytes(const HoughGeom &hg, int n_frames)
{
    return (size_t)n_frames * (hg.numangle + 2) * (size_t)(hg.numrho + 2) * sizeof(int);
}
#ifdef __HIPCC__
// THE vote of the rule: accumulator column of pixel (x, y) for one angle's table entries c, s; half = (numrho - 1) / 2.
// Three operations, each rounded to binary32 on its own, then round-half-even to int (v_rndne_f32).  The vote kernels
// and the segment walk (canny_hough_segments.hip) both call it, so the pixels of a cell are exactly those that voted.
__device__ __forceinline__ int vote_r(int x, int y, float c, float s, int half)
{
    return (int)rintf(__fadd_rn(__fmul_rn((float)x, c), __fmul_rn((float)y, s))) + half;
}
#endif
// Accumulator rows a vote workgroup keeps in LDS for a budget in bytes: at least one row if a row fits in LDS at all
// (then the budget yields), at most 16; 0 = a row does not fit, only the global-atomic form applies.
int hough_lds_rows(const HoughGeom &hg, int budget_bytes);
// vote: accum[f] = the whole (numangle + 2) x (numrho + 2) int accumulator of frame f, border included.  Source: points
// + offsets (CSR; indices >= height * width are skipped), else bits (packed, as above), else the strong plane.
// tab = numangle cosines then numangle sines (device).  lds_rows > 0: LDS rows, nothing needs zeroing; 0: the accumulator
// is zeroed, then global atomics.
hipError_t launch_hough_vote(const uint64_t *strong, const uint8_t *bits, const uint32_t *points,
                             const unsigned long long *offsets, const HystGeom &g, const HoughGeom &hg, const float *tab,
                             int *accum, int lds_rows, hipStream_t stream);
// peaks: counts[f] += peaks of frame f, hist[f * hist_bins + votes] += 1 per peak (both zeroed by the caller)
hipError_t launch_hough_peaks(const int *accum, int n_frames, const HoughGeom &hg, int threshold, int *counts,
                              unsigned *hist, int hist_bins, hipStream_t stream);
// select: the first min(lines_max, counts[f]) peaks by (votes descending, base ascending) into slot f * lines_max + k of
// lines (2 floats per slot), votes, bases (each may be null).  Workspaces: ties n_frames * numangle (zeroed by the
// caller), cut n_frames * 8 words, cand n_frames * lines_max keys.  lines_max <= kHoughMaxLines.
hipError_t launch_hough_select(const int *accum, int n_frames, const HoughGeom &hg, int threshold, int lines_max,
                               const int *counts, const unsigned *hist, int hist_bins, unsigned *ties, unsigned *cut,
                               unsigned long long *cand, float *lines, int *votes, unsigned *bases, hipStream_t stream);

// ---- Hough circles (canny_hough_circles.hip) ---------------------------
// The accumulator of a frame is (ah + 2) x (aw + 2) ints with a zero border, cells of 1 << cell_shift pixels: the shape
// convention of the line accumulator with ah for numangle and aw for numrho, so launch_hough_peaks / launch_hough_select
// find the candidate centres in it unchanged.
struct CircleGeom {
    int min_radius, max_radius, cell_shift, aw, ah;
};
constexpr int kCircleMaxRadius = 1024; // CANNY_HIP_CIRCLES_MAX_RADIUS: a radius window's squared distances stay below 2^24
constexpr int kCircleRecord = 6;       // CANNY_HIP_CIRCLE_INTS: x2, y2, radius, votes, support, base
inline size_t circles_accum_bytes(const CircleGeom &cg, int n_frames)
{
    return (size_t)n_frames * (cg.ah + 2) * (size_t)(cg.aw + 2) * sizeof(int);
}
#ifdef __HIPCC__
// The reference's 3x3 Sobel pair (calculateXYGradient) at one pixel of a frame: gx clamps columns and drops rows outside
// the frame, gy clamps rows and drops columns.  One copy for the circle votes and the edgels (canny_edgels.hip).
template <class T>
__device__ __forceinline__ void sobel_pair(const T *__restrict__ img, int h, int w, int y, int x, int *gx, int *gy)
{
    const int cl = x > 0 ? x - 1 : 0, cr = x < w - 1 ? x + 1 : w - 1;
    const int ru = y > 0 ? y - 1 : 0, rd = y < h - 1 ? y + 1 : h - 1;
    const T *row = img + (size_t)y * w, *up = img + (size_t)ru * w, *dn = img + (size_t)rd * w;
    const int ul = up[cl], uc = up[x], ur = up[cr];
    const int ml = row[cl], mr = row[cr];
    const int dl = dn[cl], dc = dn[x], dr = dn[cr];
    int v = 2 * mr - 2 * ml;
    if (y != h - 1) v += dr - dl;
    if (y != 0) v += ur - ul;
    int u = 2 * dc - 2 * uc;
    if (x != w - 1) u += dr - ur;
    if (x != 0) u += dl - ul;
    *gx = (int)(short)v;
    *gy = (int)(short)u;
}
#endif
// vote: zeroes the accumulators, then every set pixel with a non-zero gradient votes along both rays.  Source: bits (packed,
// as for the point lists) with the caller's gx / gy planes (n_frames * height * width shorts each), or else the strong plane
// with the batch's smoothed plane (bytes if smoothed_u8, else shorts), whose Sobel pair is recomputed at the set pixels.
hipError_t launch_circles_vote(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const void *smoothed,
                               bool smoothed_u8, const int16_t *gx, const int16_t *gy, const CircleGeom &cg, int *accum,
                               hipStream_t stream);
// The step arithmetic of the vote kernel alone on n pairs (the exhaustive test's hook).
hipError_t launch_circles_steps(const int16_t *gx, const int16_t *gy, size_t n, int *sx, int *sy, hipStream_t stream);
// radius: candidate k of frame f is cell bases[f * centres_max + k], k < min(centres_max, peak_counts[f]) (as
// launch_hough_select leaves them); radius / support receive its best-supported radius and that radius's pixel count.
hipError_t launch_circles_radius(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const CircleGeom &cg,
                                 const unsigned *bases, const int *peak_counts, int centres_max, int *radius, int *support,
                                 hipStream_t stream);
// accept: the candidates in order; a valid one (support > support_threshold) is accepted unless an accepted one lies within
// min_dist pixels.  circles (may be null) receives the 6-int records compactly from slot f * centres_max, counts[f] their number.
hipError_t launch_circles_accept(const HystGeom &g, const CircleGeom &cg, const unsigned *bases, const int *votes,
                                 const int *radius, const int *support, const int *peak_counts, int centres_max,
                                 int support_threshold, int min_dist, int *circles, int *counts, hipStream_t stream);

// ---- Hough line segments (canny_hough_segments.hip) --------------------
// Runs of edge pixels along detected lines.  The line list of frame f is bases[f * lines_max .. + min(lines_max,
// line_counts[f])), as launch_hough_select leaves it; tab as for the vote.  halfwin: half width of the minor-axis window a
// lane searches around its float estimate (hough_segments_halfwin); the exact vote decides inside it.
struct SegGeom {
    int numangle, numrho;
    float halfwin;
    int min_length, max_gap, lines_max, segments_max;
};
constexpr int kSegRecord = 6;                  // CANNY_HIP_SEGMENT_INTS: x0, y0, x1, y1, line, support
constexpr int kSegExclusiveMaxAxis = 1 << 20;  // exclusive mode: one bit per major position in LDS (128 KiB)
float hough_segments_halfwin(int height, int width, float rho);
// Non-exclusive, pass 1: one wave per (frame, line) walks the line and counts its segments into nseg[f * lines_max + k];
// one workgroup per frame then scans them: line_off = exclusive prefix, seg_counts[f] = the frame's total.
// Source: bits (packed, as for the point lists) or else the strong plane.
hipError_t launch_hough_segments_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg,
                                       const float *tab, const unsigned *bases, const int *line_counts, int *nseg,
                                       int *line_off, int *seg_counts, hipStream_t stream);
// Non-exclusive, pass 2: the same walk; the j-th segment of line k goes to record line_off + j of the frame if that lies
// below segments_max.
hipError_t launch_hough_segments_emit(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg,
                                      const float *tab, const unsigned *bases, const int *line_counts, const int *line_off,
                                      int *segments, hipStream_t stream);
// Exclusive: one workgroup per frame takes the lines in order on `work`, a PRIVATE copy of the source, read and cleared as
// 32-bit words with workgroup-scope atomics -- so no 32-bit word of it may hold bits of two frames.  work_is_bits: frame f's
// packed rows start at byte f * hough_segments_work_stride(g), densely packed behind that; otherwise the strong plane's words
// as they are (a frame is whole 64-bit words).  max(height, width) <= kSegExclusiveMaxAxis.
inline size_t hough_segments_work_stride(const HystGeom &g)
{
    return ((size_t)g.height * ((g.width + 7) / 8) + 127) & ~(size_t)127;
}
hipError_t launch_hough_segments_exclusive(uint32_t *work, bool work_is_bits, const HystGeom &g, const SegGeom &sg,
                                           const float *tab, const unsigned *bases, const int *line_counts, int *segments,
                                           int *seg_counts, hipStream_t stream);

// ---- Connected components (canny_components.hip) -----------------------
// Source as for the point lists: the strong plane of geometry g, or -- bits != nullptr -- a packed bit map.
// parent: n_frames * height * width ints, indexed by pixel, touched at run starts only (a run = a maximal row of set
// pixels within one 64-pixel word); it may be the label plane that launch_cc_write fills.  height * width < 2^31.
// The four launchers run in this order on one stream; their phases are described at the head of canny_components.hip.
// link: parent[s] = s, then the union of touching runs (8-connectivity) -> forest whose roots are the components' first pixels.
hipError_t launch_cc_link(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int *parent, hipStream_t stream);
// resolve: every run start points at its root; a root's entry = INT_MIN + the component's area.
hipError_t launch_cc_resolve(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int *parent,
                             hipStream_t stream);
// count: row_counts[f * height + y] = roots of that row with area >= min_area (then launch_points_scan numbers them).
hipError_t launch_cc_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *parent, int min_area,
                           uint32_t *row_counts, hipStream_t stream);
// number: every run start's entry becomes its component's number (1 .. K_f by ascending first pixel, 0 = dropped); the
// 6-int records (LEFT, TOP, WIDTH, HEIGHT, AREA, FIRST) of the numbers whose position offsets[f] + k - 1 lies below
// capacity are written into stats (may be null).
hipError_t launch_cc_number(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int *parent, int min_area,
                            const uint32_t *row_offsets, const unsigned long long *offsets, int *stats,
                            unsigned long long capacity, hipStream_t stream);
// write: labels[f][y][x] = the entry of the pixel's run start, 0 off the map (every pixel is stored); kept likewise as
// 255 / 0.  Either may be null; labels may be `entries` itself.
hipError_t launch_cc_write(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *entries, int *labels,
                           uint8_t *kept, hipStream_t stream);

// ---- Outer contour chains (canny_contours.hip) -------------------------
// Source as for the point lists.  They run behind launch_cc_link, launch_cc_resolve, launch_cc_count and
// launch_points_scan on the same stream and BEFORE launch_cc_number (which replaces the roots' entries): parent is as
// resolve leaves it, row_offsets / offsets are the record CSR of the scan.  height * width <= kContourMaxPixels: a chain has
// at most 8 * area + 1 points, and the per-frame sums of the scan are 32-bit.
constexpr long long kContourMaxPixels = 1ll << 28;
// count: every kept component's border is followed once; chain_offsets[j + 1] = the length of record j's chain for
// j < capacity (chain_offsets may be null: capacity counts as 0), chain_offsets[0] = 0, row_points[f * height + y] = chain
// points of ALL kept components whose first pixel lies in that row (then launch_points_scan gives point_offsets).
hipError_t launch_ct_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *parent, int min_area,
                           const uint32_t *row_offsets, const unsigned long long *offsets,
                           unsigned long long *chain_offsets, unsigned long long capacity, uint32_t *row_points,
                           hipStream_t stream);
// place: the lengths in chain_offsets[1 .. min(K, capacity)] become prefix sums over the whole batch (in place).
hipError_t launch_ct_place(const HystGeom &g, const uint32_t *row_offsets, const unsigned long long *offsets,
                           const uint32_t *row_point_offsets, const unsigned long long *point_offsets,
                           unsigned long long *chain_offsets, unsigned long long capacity, hipStream_t stream);
// write: the same walks; points[chain_offsets[j] + i] = the i-th pixel (r * width + c) of record j's chain, for j < capacity
// and positions below point_capacity; nothing is stored at or beyond points + point_capacity.
hipError_t launch_ct_write(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *parent, int min_area,
                           const uint32_t *row_offsets, const unsigned long long *offsets,
                           unsigned long long *chain_offsets, unsigned long long capacity, int *points,
                           unsigned long long point_capacity, hipStream_t stream);

// ---- Edge curves (canny_curves.hip) -------------------------------------
// Source as for the point lists.  height * width <= kContourMaxPixels: a frame has at most 4 points per pixel and 2 curves
// per pixel, and the per-frame sums of the scan are 32-bit.
// count: row_curves[f * height + y] / row_points[f * height + y] = the kept curves (at least min_length points) that start
// in that row / their points; every row's word is written (then launch_points_scan on each gives offsets / point_offsets).
hipError_t launch_cv_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_length,
                           uint32_t *row_curves, uint32_t *row_points, hipStream_t stream);
// write: behind the two scans; chain_offsets[0] = 0, chain_offsets[j + 1] = the end of record j's points and records[4 * j
// ..] (records may be null) for j < capacity (>= 1, chain_offsets not null), points[chain_offsets[j] + i] = the curve's i-th
// pixel for positions below point_capacity (points may be null); nothing is stored past either capacity.
hipError_t launch_cv_write(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_length,
                           uint32_t *row_curves, uint32_t *row_points, const unsigned long long *offsets,
                           const unsigned long long *point_offsets, unsigned long long *chain_offsets,
                           unsigned long long capacity, int *records, int *points, unsigned long long point_capacity,
                           hipStream_t stream);

// ---- Polygon approximation of the chains (canny_polygons.hip) ----------
// They read what a contours call stored: offsets (the record CSR, only offsets[n_frames] is used), chain_offsets and points.
// R = min(offsets[n_frames], capacity) is read on the device.  height, width <= kPolygonMaxSide keep every cross product
// below 2^31.  masks: capacity u64; flags: point_capacity bytes; block_sums: polygons_scan_blocks(capacity) u64.
constexpr int kPolygonMaxSide = 32768;
unsigned long long polygons_scan_blocks(unsigned long long capacity);
// simplify: vertex_offsets[0] = 0, vertex_offsets[j + 1] = the vertex count of record j (0 for a chain cut by
// point_capacity); the vertex set goes to masks[j] (chains of at most 64 points) or flags[chain_offsets[j] + i];
// measures (may be null) [j][0 .. 1] = vertices, length_q8, and (-1, 0, 0, 0) for a cut chain.
hipError_t launch_pg_simplify(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                              const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity,
                              int width, unsigned epsilon_q8, unsigned ratio_q16, unsigned long long *vertex_offsets,
                              unsigned long long *masks, uint8_t *flags, long long *measures, hipStream_t stream);
// scan: vertex_offsets[1 .. R] become inclusive prefix sums, in place.
hipError_t launch_pg_scan(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                          unsigned long long *vertex_offsets, unsigned long long *block_sums, hipStream_t stream);
// emit: vertices[vertex_offsets[j] + rank] below vertex_capacity (vertices may be null with capacity 0);
// measures (may be null) [j][2 .. 3] = area2, convex of the complete records.
hipError_t launch_pg_emit(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                          const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity,
                          int width, const unsigned long long *vertex_offsets, const unsigned long long *masks,
                          const uint8_t *flags, int *vertices, unsigned long long vertex_capacity, long long *measures,
                          hipStream_t stream);

// ---- contour shape measures (canny_shapes.hip) --------------------------
// Same inputs as the polygon stage.  height, width <= kShapeMaxSide keep every coordinate in 15 bits.  ws: shapes_ws_ints
// (point_capacity) ints, five arrays of point_capacity ints each, indexed like points: the smallest and the largest y per
// column of a chain's bounding box, the two lists of the hull's rounds, and the finished hull packed (y << 16 | x).
constexpr int kShapeMaxSide = 32767;
inline size_t shapes_ws_ints(unsigned long long point_capacity) { return 5 * (size_t)point_capacity; }
// measure: hull_offsets[0] = 0, hull_offsets[j + 1] = V_h of record j (0 for a cut chain); the hull goes to the workspace;
// measures (may be null) [j][0 .. 13], and (-1, 0, ...) for a cut chain.
hipError_t launch_sh_measure(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                             const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity,
                             int width, unsigned long long *hull_offsets, int *ws, long long *measures, hipStream_t stream);
// emit (behind launch_pg_scan on hull_offsets): hull[hull_offsets[j] + k] below hull_capacity (hull may be null with
// capacity 0); measures (may be null) [j][14 .. 19] of the complete records.
hipError_t launch_sh_emit(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                          const unsigned long long *chain_offsets, unsigned long long point_capacity, int width,
                          const unsigned long long *hull_offsets, const int *ws, int *hull, unsigned long long hull_capacity,
                          long long *measures, hipStream_t stream);

// ---- Euclidean distance transform (canny_edt.hip) ----------------------
// Source as for the point lists.  height * width < 2^31 and height^2 + width^2 < 2^31.
// Elements per row of the u16 plane between the two passes: rows are padded to whole 64-pixel words.
inline size_t edt_pitch(const HystGeom &g) { return (size_t)g.tiles_x << 6; }
// rows: cols[f][r][c] = the column of the set pixel of row r nearest to column c (ties to the left), 0xFFFF if the row has
// none.  cols holds n_frames * height * edt_pitch(g) u16.
hipError_t launch_edt_rows(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, uint16_t *cols,
                           hipStream_t stream);
// columns: the lower envelope of the rows' parabolas down every column -> dist2, dist, nearest ([n][height][width]; any may
// be null, every element of the others is stored).  cols is consumed (it becomes part of the scan's stack).  stack:
// n_frames * height * edt_pitch(g) u32, or null when dist2 is given -- the scan then keeps its stack in dist2.
hipError_t launch_edt_columns(const HystGeom &g, uint16_t *cols, uint32_t *stack, int *dist2, float *dist, int *nearest,
                              hipStream_t stream);

// ---- Sub-pixel edgels (canny_edgels.hip) --------------------------------
// Records are 4 ints (CANNY_HIP_EDGEL_INTS), 16-byte aligned.  plane: n_frames contiguous height x width planes, bytes if
// plane_u8 else shorts.
// rows: behind launch_points_count / launch_points_scan of the same strong plane on the same stream; record
// offsets[f] + row_offsets[f * height + y] + k describes the k-th set column of the row, for every position below
// capacity; points (optional) receives y * width + column at the same position.  The grid is plan_points_rows' rows at
// four waves a workgroup.
hipError_t launch_edgels_rows(const uint64_t *strong, const HystGeom &g, const void *plane, bool plane_u8,
                              const uint32_t *row_offsets, const unsigned long long *offsets, int *edgels,
                              uint32_t *points, unsigned long long capacity, hipStream_t stream);
// at: record q describes pixel index points[q] of the frame f with offsets[f] <= q < offsets[f + 1], for q < capacity;
// an index >= height * width gives the invalid record and is never dereferenced.
hipError_t launch_edgels_at(const void *plane, bool plane_u8, int height, int width, int n_frames, const uint32_t *points,
                            const unsigned long long *offsets, int *edgels, unsigned long long capacity,
                            hipStream_t stream);
// The arithmetic of the kernels alone (the exhaustive test's hook): pairs -> mag_q4, dir; (a, b, c) triples -> t_q8, refined.
hipError_t launch_edgels_arith(const int16_t *gx, const int16_t *gy, size_t n_pairs, uint32_t *mag, int *dir,
                               const uint32_t *abc, size_t n_triples, int *t, int *refined, hipStream_t stream);

// ---- Sub-pixel line fits (canny_line_fits.hip) ---------------------------
// One 12-int record (CANNY_HIP_LINE_FIT_INTS) per segment slot f * segments_max + j, j < min(segments_max, seg_counts[f]),
// from the records launch_hough_segments_* left in `segments`; source (bits or else the strong plane), tab, bases and
// line_counts as there; of sg only numangle, numrho, halfwin, lines_max and segments_max are read.  plane: n_frames
// contiguous height x width planes, bytes if plane_u8 else shorts.  Grid (ceil(segments_max / 4), n_frames): no cap.
hipError_t launch_line_fits(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const SegGeom &sg,
                            const float *tab, const unsigned *bases, const int *line_counts, const int *segments,
                            const int *seg_counts, const void *plane, bool plane_u8, int options, int *fits,
                            hipStream_t stream);
// The finishing arithmetic alone (the test hook): n sets of 8 long longs -> 6 ints each; one lane per set, no cap.
hipError_t launch_line_fits_arith(const long long *moments, size_t n, int *out, hipStream_t stream);

// ---- Sub-pixel circle fits (canny_circle_fits.hip) -----------------------
// One 8-int record (CANNY_HIP_CIRCLE_FIT_INTS) per circle slot f * centres_max + j, j < min(centres_max, counts[f]), from
// the 6-int records launch_circles_accept (or the caller) left in `circles`; source (bits or else the strong plane) as for
// the line fits.  plane: n_frames contiguous height x width planes, bytes if plane_u8 else shorts.  fits: 16-byte aligned.
// Grid (centres_max, n_frames), one workgroup per slot: no cap.
hipError_t launch_circle_fits(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *circles,
                              const int *counts, int centres_max, const void *plane, bool plane_u8, int band, int trim_q8,
                              int options, int *fits, hipStream_t stream);
// The finishing arithmetic alone (the test hook): n sets of 12 long longs -> 4 ints each; one lane per set, no cap.
hipError_t launch_circle_fits_arith(const long long *moments, size_t n, int *out, hipStream_t stream);
// Pixels of one record that the kernel's LDS queue holds (the rest is recomputed in every pass).
int circle_fits_queue_capacity();

// ---- launch plans of the capped grids ---------------------------------
// A launcher whose grid is capped hands its kernel `units` work items and `grid` workgroups that take `per_group` items
// per trip of their grid-stride loop.  Each plan_* below is computed from sizes alone, is THE grid computation of the
// launchers named beside it (they launch plan.grid workgroups), and is what canny_hip_selftest_launch_plan reports: a
// test asks it whether a call sends some wave into a second trip.
struct LaunchPlan {
    unsigned long long units; // work items of the launch (of one frame where the grid's y is the frame)
    unsigned per_group;       // items one workgroup takes per trip
    unsigned grid;            // workgroups (x)
    int aux;                  // plan_edt_rows: rows per wave; otherwise 0
    unsigned long long trips() const
    {
        const unsigned long long per_trip = (unsigned long long)grid * per_group;
        return (units + per_trip - 1) / per_trip;
    }
};
// The kernel walks `units` items, per_group a workgroup and trip; grid = ceil(sizing / per_sizing), at least 1 and at most
// cap -- for the launches whose grid is sized by another figure than what their loop walks.
inline LaunchPlan sized_plan(unsigned long long units, unsigned per_group, unsigned long long sizing, unsigned per_sizing,
                             unsigned cap, int aux = 0)
{
    const unsigned long long want = (sizing + per_sizing - 1) / per_sizing;
    return LaunchPlan{units, per_group, (unsigned)(want < 1 ? 1 : (want > cap ? cap : want)), aux};
}
// grid = ceil(units / per_group), at least 1 and at most cap
inline LaunchPlan capped_plan(unsigned long long units, unsigned per_group, unsigned cap, int aux = 0)
{
    return sized_plan(units, per_group, units, per_group, cap, aux);
}
LaunchPlan plan_points_rows(const HystGeom &g);    // points count, scatter: image rows of the batch
LaunchPlan plan_scan_frames(int n_frames);         // points_scan_frames_kernel: frames, one workgroup
LaunchPlan plan_cc_tiles(const HystGeom &g);       // cc init, merge, flatten, area, relabel, write: tiles of the batch
LaunchPlan plan_cc_rows(const HystGeom &g);        // cc count, number: image rows of the batch
LaunchPlan plan_cc_fixup(unsigned long long capacity); // cc_fixup_kernel: record slots
LaunchPlan plan_ct_rows(const HystGeom &g);        // contour walk (count, write), place: image rows of the batch
LaunchPlan plan_cv_rows(const HystGeom &g);        // curve walks (count, write): image rows of the batch
LaunchPlan plan_edt_rows(const HystGeom &g);       // edt rows: groups of aux consecutive rows
LaunchPlan plan_edt_columns(const HystGeom &g);    // edt columns: 64-column strips of the batch
LaunchPlan plan_pg_records(unsigned long long capacity);   // polygon simplify, emit: record slots
LaunchPlan plan_pg_scan_sums(unsigned long long capacity); // pg_scan_sums_kernel: chunk sums, one workgroup
LaunchPlan plan_sh_records(unsigned long long capacity);   // shape measure, emit: record slots
// global vote: the items of a frame as the kernel walks them -- the plane's words (tile padding included for the strong
// plane; a trip is one word per lane, and a lane keeps four in flight) or the n_points points of the frame's list (only
// the query knows them: the grid is sized by pixels / 16, and by the strong plane's words for both plane sources)
enum VoteSource { kSrcStrong = 0, kSrcBits = 1, kSrcPoints = 2 };
LaunchPlan plan_hough_vote_global(const HystGeom &g, VoteSource src, unsigned long long n_points = 0);
LaunchPlan plan_hough_cells(unsigned long long cells);    // peaks, ties, collect: the numangle * numrho cells of a frame
LaunchPlan plan_circles_vote(const HystGeom &g, bool from_bits); // circle vote: 64-word chunks of a frame
LaunchPlan plan_circles_steps(size_t n);           // circles_steps_kernel: gradient pairs
LaunchPlan plan_to_gray(size_t n_px);              // to_gray_kernel: 16-pixel groups
// edgels_at_kernel: the n_points points of a frame's list; the grid is sized by the frame's pixels / 1024 (only the device
// knows the lists).  edgels_arith_kernel: pairs or triples.  (Reported by canny_hip_selftest_edgels_plan, not by a kind.)
LaunchPlan plan_edgels_at(int height, int width, unsigned long long n_points);
LaunchPlan plan_edgels_arith(size_t n);

// ---- chamfer template matching (canny_chamfer.hip) ----------------------
// A template set as the kernels read it: the points of every template sorted by (dy, dx) and packed (dx in the low half,
// dy in the high half of a word), per template its bounding box, and the bands of dy the tiled kernel walks: the points
// [begin, end) of a band lie in rows dy0 .. dy0 + rows - kChamferTileY of the template, and rows * cols(t) u16 fit in LDS.
constexpr int kChamferTileX = 64, kChamferTileY = 16; // anchors of one workgroup: a lane per column, 4 rows per lane
constexpr int kChamferLdsElems = 32768;               // u16 elements of the tile with its halo: 64 KiB
struct ChamferBox {
    int min_x, max_x, min_y, max_y;
};
struct ChamferBand {
    int begin, end, dy0, rows;
};
struct ChamferLayout {
    int n_templates = 0;
    std::vector<int> offsets;      // T + 1
    std::vector<uint32_t> points;  // packed, sorted per template
    std::vector<ChamferBox> boxes; // T
    std::vector<int> band_offsets; // T + 1
    std::vector<ChamferBand> bands;
    int max_elems = 0;             // the largest rows * cols of any band
    int max_k = 0;                 // the largest K_t
};
// Validates host template arrays (0 ok, 1 invalid, 2 unsupported: the values of CANNY_HIP_ERR_*) and lays them out.
int chamfer_build_layout(const int *offsets, const short *points, int n_templates, ChamferLayout &out);
// The route the automatic choice takes for a layout: 1 direct, 2 tiled.
int chamfer_auto_route(const ChamferLayout &lay);
struct ChamferSetDev { // device copies of a layout
    const int *offsets;
    const uint32_t *points;
    const ChamferBox *boxes;
    const int *band_offsets;
    const ChamferBand *bands;
    int n_templates, max_elems;
};
LaunchPlan plan_chamfer_cost(unsigned long long n_px);   // cost pass: pixels of the chunk
LaunchPlan plan_chamfer_cells(unsigned long long cells); // direct score, histogram, collect: the T * h * w anchors of a frame
// Frames of one chunk of the batch: at most 4096, and as many as keep the larger workspace of the chunk -- the scores, or
// with the caller's score plane the u16 costs -- within budget_mb MiB (0: 256), one frame at least.
int chamfer_chunk_frames(int n_frames, int height, int width, int n_templates, bool with_scores, int budget_mb = 0);
// The candidate passes' workspace for a chunk of nf frames: histogram | state | collect counters | keys.
size_t chamfer_ws_bytes(int nf, int matches_max);
// cost: dist2 (n_px ints) -> u16 costs.  costs_hook: the same arithmetic (trunc_q4 >= 1) or the untruncated root (0) as u32.
hipError_t launch_chamfer_cost(const int *dist2, size_t n_px, int trunc_q4, uint16_t *cost, hipStream_t stream);
hipError_t launch_chamfer_costs_hook(const int *dist2, size_t n, int trunc_q4, unsigned *out, hipStream_t stream);
// score: scores[f][t][y][x] for the nf frames of cost.  tiled: the LDS route, else one lane per anchor.
hipError_t launch_chamfer_score(const uint16_t *cost, int nf, int height, int width, const ChamferSetDev &set, int trunc_q4,
                                bool tiled, unsigned *scores, hipStream_t stream);
// candidates + accept of nf frames: local minima under the threshold, the matches_max smallest keys (radix select over four
// digit passes, then collect), sort and ordered acceptance.  ws: chamfer_ws_bytes(nf, matches_max), zeroed here.  matches,
// counts, cand_counts: already offset to the chunk's first frame; matches and cand_counts may be null.
hipError_t launch_chamfer_candidates(const unsigned *scores, int nf, int height, int width, const ChamferSetDev &set,
                                     int max_mean_q4, int matches_max, void *ws, int *cand_counts, hipStream_t stream);
hipError_t launch_chamfer_accept(const unsigned *scores, int nf, int height, int width, int n_templates, int matches_max,
                                 int min_dist, void *ws, int *matches, int *counts, hipStream_t stream);

// ---- corners, Harris / Shi-Tomasi (canny_corners.hip) --------------------
struct CornerArgs { // validated by the caller: the ranges of include/canny_hip.h
    int mode, block, k_q8, quality_q16;
    long long min_response;
    int min_dist, corners_max;
};
constexpr int kCornersChunk = 1024; // frames of one chunk of the batch (the grid's y)
// max, candidates (histograms), collect: the 64 x 16 tiles of ONE frame, one per workgroup and trip.  arith: triples.
// (Reported by canny_hip_selftest_corners_plan, not by a kind.)
LaunchPlan plan_corners_tiles(int height, int width);
LaunchPlan plan_corners_arith(size_t n);
// The workspace of a chunk of nf frames: keys | key lists | prefix, cutoff | maxima | histogram | state | counters.
size_t corners_ws_bytes(int nf, int corners_max, int height, int width);
// The four parts, in this order, for the nf <= kCornersChunk frames of plane (bytes if plane_u8, else shorts in [0, 255]).
// max zeroes what the call reads before writing (the rest of ws is written first); response (may be null) receives every R.
// cand_counts, max_response (may be null), corners, counts: already offset to the chunk's first frame.
hipError_t launch_corners_max(const void *plane, bool plane_u8, int nf, int height, int width, const CornerArgs &a, void *ws,
                              long long *response, hipStream_t stream);
hipError_t launch_corners_candidates(const void *plane, bool plane_u8, int nf, int height, int width, const CornerArgs &a,
                                     void *ws, int *cand_counts, long long *max_response, hipStream_t stream);
hipError_t launch_corners_collect(const void *plane, bool plane_u8, int nf, int height, int width, const CornerArgs &a,
                                  void *ws, hipStream_t stream);
hipError_t launch_corners_accept(int nf, int height, int width, const CornerArgs &a, void *ws, long long *corners,
                                 int *counts, hipStream_t stream);
// The response function alone on n triples (sxx, syy, sxy): the arithmetic test's hook.
hipError_t launch_corners_arith(const int *sums, size_t n, int mode, int k_q8, long long *out, hipStream_t stream);

// ---- corner descriptors and Hamming matching (canny_descriptors.hip) --------------------
// describe: the n_frames * corners_max record slots, four (one a wave) per workgroup and trip.  match, reverse: the
// (pair, block of 256 descriptors of the register side) units, one per workgroup and trip.  (Reported by
// canny_hip_selftest_descriptors_plan, not by a kind.)
LaunchPlan plan_desc_slots(unsigned long long slots);
LaunchPlan plan_desc_match(unsigned long long n_pairs, int stride);
// Descriptors of the records (4 long long a slot, slot f * corners_max + j, j < counts[f]) on plane (bytes if plane_u8, else
// shorts in [0, 255]): desc 4 words and meta one int per slot; slots past counts[f] are not written.
hipError_t launch_desc_describe(const void *plane, bool plane_u8, int n_frames, int height, int width,
                                const long long *corners, const int *counts, int corners_max, int steered,
                                unsigned long long *desc, int *meta, hipStream_t stream);
// Best and second-best neighbour of every descriptor of the q side among the t side's, per pair (pairs: device, 2 ints a
// pair: q frame, t frame).  !reverse: out [n_pairs][stride_q][4] receives j, d1, d2.  reverse: the caller passes the train
// set as q and the query set as t, the pairs are read the other way round, out [n_pairs][stride_q] receives j.
hipError_t launch_desc_match(const unsigned long long *q_desc, const int *q_counts, int stride_q,
                             const unsigned long long *t_desc, const int *t_counts, int stride_t, const int *pairs,
                             int n_pairs, bool reverse, int *out, hipStream_t stream);
// The flags (word 3 of every match) and the accepted matches of each pair; back is the reverse launch's output.
hipError_t launch_desc_finalize(const int *q_counts, int stride_q, int stride_t, const int *pairs, int n_pairs,
                                const int *back, int max_distance, int ratio_q8, int cross, int *matches, int *pair_counts,
                                hipStream_t stream);

// ---- frame-to-frame motion from the corner matches (canny_motion.hip) --------------------
// gather, refit: the pairs, one per workgroup and trip.  score: the (pair, block of 256 hypotheses) units, one per workgroup
// and trip.  (Reported by canny_hip_selftest_motion_plan, not by a kind.)
LaunchPlan plan_motion_pairs(unsigned long long n_pairs);
LaunchPlan plan_motion_score(unsigned long long n_pairs, int hypotheses);
// The workspace of one call, carved from `base` (8-byte aligned; a NULL base gives the size alone): per (pair, query slot) the
// compacted correspondence (four u16) and its slot, per (pair, hypothesis) its inlier count, per pair m, then the pairs
// (device copy, 2 ints a pair: the caller uploads them before the gather).
struct MotionWs {
    void *list;
    int *slot, *counts, *m, *pairs;
    size_t bytes;
};
MotionWs motion_workspace(void *base, int n_pairs, int stride_q, int hypotheses);
// The correspondences of every pair in query order, m, and (inlier != NULL) the -1 flags of the other slots below the count.
hipError_t launch_motion_gather(const long long *q_corners, const int *q_counts, int stride_q, const long long *t_corners,
                                const int *t_counts, int stride_t, int n_pairs, const int *matches, const MotionWs &w,
                                int *inlier, hipStream_t stream);
// The inlier count of every (pair, hypothesis); -1 where the hypothesis is invalid.
hipError_t launch_motion_score(int stride_q, int n_pairs, int model, int thr_q4, int hypotheses, unsigned seed,
                               const MotionWs &w, hipStream_t stream);
// The best hypothesis, the flags of the correspondences, the refit and the 16-word record of every pair.
hipError_t launch_motion_refit(int stride_q, int n_pairs, int model, int thr_q4, int hypotheses, unsigned seed,
                               const MotionWs &w, long long *motion, int *inlier, hipStream_t stream);

// ---- frame alignment: the motions chained, frames warped (canny_warp.hip) --------------
// warp: the n_out * ceil(out_h / 16) * ceil(out_w / 64) output tiles, one per workgroup and trip.  (Reported by
// canny_hip_selftest_warp_plan, not by a kind.)
LaunchPlan plan_warp_tiles(int n_out, int out_h, int out_w);
// What the tiled route does with tile (tile_x, tile_y) of a frame warped by the record `xform` (8 words; its source index is
// not looked at): true if the footprint is staged in LDS; box: the clipped footprint x0, y0, x1, y1 (empty: x1 < x0).
bool warp_tile_footprint(const long long *xform, int interp, int src_h, int src_w, int out_h, int out_w, int tile_x,
                         int tile_y, int box[4]);
// n_pairs + 1 transform records from the motion records of the consecutive pairs; one lane.
hipError_t launch_warp_compose(const long long *motion, int n_pairs, int first_frame, long long *xforms, hipStream_t stream);
// Every output byte and (valid != NULL) every valid byte.  route: 0 automatic, 1 direct, 2 tiled.
hipError_t launch_warp_frames(const uint8_t *src, int n_src, int src_h, int src_w, const long long *xforms, int n_out,
                              int out_h, int out_w, int interp, int border, int route, uint8_t *out, uint8_t *valid,
                              hipStream_t stream);

// ---- temporal fusion of aligned frames and change masks (canny_fuse.hip) ----------------
// fuse: the n_groups * ceil(h / 16) * ceil(w / 64) output tiles, one per workgroup and trip; the change mask: the same with
// its n_frames.  (Reported by canny_hip_selftest_fuse_plan, not by a kind.)
LaunchPlan plan_fuse_tiles(int n_planes, int h, int w);
// The route a MEDIAN of group_len frames takes under the option value `route` (0 automatic, 1 registers, 2 passes): 1 or 2.
int fuse_median_route(int group_len, int route);
// Every byte of fused [n_groups][h][w] and (count != NULL) of count.  valid may be NULL: every pixel is valid.
hipError_t launch_fuse_frames(const uint8_t *frames, const uint8_t *valid, int n_frames, int h, int w, int group_len,
                              int group_step, int op, int fill, int min_count, int route, uint8_t *fused, uint8_t *count,
                              hipStream_t stream);
// Every byte of mask [n_frames][h][ceil(w / 8)]; changed (may be NULL, 8-byte aligned) is zeroed on the stream, then summed.
hipError_t launch_change_mask(const uint8_t *frames, const uint8_t *valid, int n_frames, int h, int w, const uint8_t *bg,
                              const uint8_t *bg_count, int per_bg, int thr, int min_count, uint8_t *mask,
                              unsigned long long *changed, hipStream_t stream);
// canny_hip_selftest_fuse_mean: the kernels' rounded mean over every (c, s) into table [255][65026], unused cells 0.
hipError_t launch_fuse_mean_table(uint8_t *table, hipStream_t stream);

// ---- binary morphology on packed bit maps (canny_morph.hip) ------------------------------
// One primitive step is one launch over the n_frames * ceil(h / 64) * ceil(ceil(w / 64) / 8) tiles of 8 words x 64 rows, one
// per workgroup and trip.  (Reported by canny_hip_selftest_morph_plan, not by a kind.)
LaunchPlan plan_morph_tiles(int n_frames, int h, int w);
// The route automatic takes for a full rectangle of kw x kh: 1 general, 2 separable.
int morph_auto_route(int kw, int kh);
// Every byte of out [n_frames][h][ceil(w / 8)], pad bits 0.  src: a packed map of that layout or -- src_plane -- the strong
// bit-plane of make_hyst_geom(h, w, n_frames).  op, border: the header's enums; rows[kh]: host memory, read before the call
// returns; route: 0 automatic, 1 general, 2 separable (full rectangles only).  ws_a, ws_b: two maps of out's size for the
// intermediates of more than one (ws_a) or two (ws_b) primitive steps; out itself holds intermediates of GRADIENT.  counts
// (may be NULL, 8-byte aligned) is zeroed on the stream, then summed by the last step.
hipError_t launch_morph(const void *src, bool src_plane, int n_frames, int h, int w, int op, const unsigned *rows, int kw,
                        int kh, int border, int iterations, int route, uint8_t *ws_a, uint8_t *ws_b, uint8_t *out,
                        unsigned long long *counts, hipStream_t stream);

// ---- binarization: gray planes to packed bit maps (canny_binarize.hip) -------------------
// plane: [n_frames][h][w] bytes (in_u8) or shorts in [0, 255]; out: every byte of [n_frames][h][ceil(w / 8)], pad bits 0.
// counts (may be NULL, 8-byte aligned) is zeroed on the stream, then summed by the kernel that writes the bits.
// The map of FIXED and OTSU: bit = (v > thr[f]) != invert; 256 output bytes per workgroup and trip.
LaunchPlan plan_binarize_bytes(int n_frames, int h, int w);
hipError_t launch_binarize_map(const void *plane, bool in_u8, int n_frames, int h, int w, const int *thr, int invert,
                               uint8_t *out, unsigned long long *counts, hipStream_t stream);
// One workgroup per frame: Otsu's threshold (the header's integer rule) of hist[f][kHistBins] -> thr[f].
hipError_t launch_binarize_otsu(const uint32_t *hist, int n_frames, int *thr, hipStream_t stream);
// ADAPTIVE_MEAN: bit = (2 S < kw kh (2 (v + c) - 1)) != invert, S the clamped kw x kh window sum.  route 1: every lane sums
// its windows from global memory (plan_binarize_bytes); route 2: a wave marches down a strip of binarize_strip_cols()
// useful columns, binarize_segment_rows(kh) rows a segment (plan_binarize_march); 0: binarize_auto_route(kw, kh).
LaunchPlan plan_binarize_march(int n_frames, int h, int w, int kh);
int binarize_strip_cols();
int binarize_segment_rows(int kh);
int binarize_staged_cols(int kw); // the strip and the halo a wave has room for: 64 lanes x 9 or 13 columns
int binarize_auto_route(int kw, int kh);
hipError_t launch_binarize_adaptive(const void *plane, bool in_u8, int n_frames, int h, int w, int c, int kw, int kh,
                                    int invert, int route, uint8_t *out, unsigned long long *counts, hipStream_t stream);

// ---- thinning of packed bit maps (canny_thin.hip) ------------------------------------------
// Every launch of a call walks the n_frames * ceil(h / 64) * ceil(ceil(w / 64) / 8) tiles of 8 words x 64 rows, one per
// workgroup and trip.  (Reported by canny_hip_selftest_thin_plan, not by a kind.)
LaunchPlan plan_thin_tiles(int n_frames, int h, int w);
int thin_auto_fuse();  // the full iterations a launch of the automatic route runs; 0: automatic is the stepwise route
// The context workspace of a call: two maps | the deletions per frame and iteration of two chunks | the frames' states | a word
size_t thin_workspace_bytes(int n_frames, int h, int w);
// A call is zero, passes, info on one stream.  src: a packed map [n_frames][h][ceil(w / 8)] or -- src_plane -- the strong
// bit-plane of make_hyst_geom(h, w, n_frames); out: every byte of a packed map, pad bits 0.  method, max_iterations: the
// header's; route: 0 automatic, 1 stepwise, 2 fused; fuse: 0 automatic, 1..8.  max_iterations = 0 synchronises the stream
// between chunks of launches.  info (may be NULL, 8-byte aligned): 4 long long a frame.
hipError_t launch_thin_zero(void *ws, int n_frames, int h, int w, long long *info, hipStream_t stream);
hipError_t launch_thin_passes(const void *src, bool src_plane, int n_frames, int h, int w, int method, int max_iterations,
                              int route, int fuse, void *ws, uint8_t *out, hipStream_t stream);
hipError_t launch_thin_info(void *ws, int n_frames, int h, int w, int max_iterations, long long *info, hipStream_t stream);

// ---- morphological reconstruction of packed bit maps (canny_reconstruct.hip) ---------------
// The sweep launches of a call.  route 2 (and 0 where automatic is the tile flood): the n_frames * ceil(h / 64) *
// ceil(ceil(w / 64) / 8) tiles of 8 words x 64 rows, one per workgroup and trip; route 1: the n_frames * h * ceil(w / 64)
// words, 256 per workgroup and trip.  Init and finish have the plan of route 1.  (Reported by
// canny_hip_selftest_reconstruct_plan, not by a kind.)
LaunchPlan plan_reconstruct(int n_frames, int h, int w, int route);
int reconstruct_auto_route(); // 1 stepwise or 2 tile flood
// What a call needs of the context's thin_ws: a word-aligned copy of the state | the changed words of two chunks of launches
// | three accumulators a frame | the poll word
size_t reconstruct_workspace_bytes(int n_frames, int h, int w);
// A call is the three phases in this order with the same arguments on one stream.  marker: a packed map
// [n_frames][h][ceil(w / 8)] for op 0, NULL otherwise; mask: a packed map or -- mask_plane -- the strong bit-plane of
// make_hyst_geom(h, w, n_frames); out: every byte of a packed map, pad bits 0; between the phases it (or the workspace, where
// its rows are not whole aligned words) holds the flood's state.  op, connectivity: the header's; route: 0 automatic,
// 1 stepwise, 2 tile flood.  SWEEPS synchronises the stream behind every chunk of launches and reports the sweep launches it
// queued in *launches; FINISH synchronises it once more.  info (may be NULL, 8-byte aligned): 3 long long a frame.
enum { RECON_INIT = 0, RECON_SWEEPS = 1, RECON_FINISH = 2 };
hipError_t launch_reconstruct(int phase, const uint8_t *marker, const void *mask, bool mask_plane, int n_frames, int h, int w,
                              int op, int connectivity, int route, void *ws, uint8_t *out, long long *info, int *launches,
                              hipStream_t stream);

// ---- grey-level morphology and median filtering of u8 planes (canny_gray_morph.hip) ---------
// One primitive step is one launch over the n_frames * ceil(h / 32) * ceil(w / 128) tiles of 128 columns x 32 rows, one per
// workgroup and trip.  (Reported by canny_hip_selftest_gray_morph_plan, not by a kind.)
LaunchPlan plan_gray_morph_tiles(int n_frames, int h, int w);
// The route automatic takes for op (the header's enum) with a full rectangle of kw x kh: 1 general, 2 fast.
int gray_morph_auto_route(int op, int kw, int kh);
// Every byte of out [n_frames][h][w].  src: a plane of bytes or -- src_s16 -- of shorts in [0, 255].  op, border_mode: the
// header's enums; rows[kh]: host memory, read before the call returns; route: 0 automatic, 1 general, 2 fast (full rectangles
// and the median).  ws_a, ws_b: two planes of out's size for the intermediates of more than one (ws_a) or two (ws_b)
// primitive steps; out itself holds intermediates of GRADIENT.
hipError_t launch_gray_morph(const void *src, bool src_s16, int n_frames, int h, int w, int op, const unsigned *rows, int kw,
                             int kh, int border_mode, int border_value, int iterations, int route, uint8_t *ws_a, uint8_t *ws_b,
                             uint8_t *out, hipStream_t stream);

// ---- image pyramids of u8 planes: pyrDown and pyrUp (canny_pyramid.hip) ---------------------
// Every launch walks the n_frames * ceil(out_h / 32) * ceil(out_w / 128) tiles of 128 columns x 32 rows of its OUTPUT, one per
// workgroup and trip.  (Reported by canny_hip_selftest_pyramid_plan, not by a kind.)
LaunchPlan plan_pyramid_tiles(int n_frames, int out_h, int out_w);
// The route automatic takes for pyrDown: 1 direct, 2 tiled.  It depends on nothing.
int pyramid_auto_route();
// Every byte of out [n_frames][(h + 1) / 2][(w + 1) / 2].  src: a plane [n_frames][h][w] of bytes or -- src_s16 -- of shorts
// in [0, 255]; route: 0 automatic, 1 direct, 2 tiled.  One launch.
hipError_t launch_pyr_down(const void *src, bool src_s16, int n_frames, int h, int w, int route, uint8_t *out, hipStream_t stream);
// Every byte of out [n_frames][oh][ow], oh in {2 h - 1, 2 h}, ow in {2 w - 1, 2 w}.  One launch.
hipError_t launch_pyr_up(const uint8_t *src, int n_frames, int h, int w, int oh, int ow, uint8_t *out, hipStream_t stream);

// ---- measurement aid ------------------------------------------------------------------------
// Plain device copy of nbytes (multiple of 16; both pointers 16-byte aligned): what a 1:1 read/write stream reaches.
hipError_t launch_probe_copy(const void *src, void *dst, size_t nbytes, hipStream_t stream, const LaunchEvents &ev = {});

// ---- self-test ------------------------------------------------------------------------------
hipError_t launch_selftest_mag_angle(int lim, int16_t *mags, uint8_t *bins, hipStream_t stream);
// The marching kernels' per-pixel helpers (canny_sobel_nms_march.hip); form as canny_hip_selftest_sobel_pixel, 1..3.
hipError_t launch_selftest_sobel_pixel(int form, int lim, int16_t *mags, uint8_t *bins, hipStream_t stream);
// Counts floats a (bit patterns first_bits..last_bits) for which the Gaussian's reciprocal-based
// division a/b differs from the IEEE divide; *d_mismatches must be zero beforehand.
// use_fma != 0 checks the one-instruction form fma(a, c, a) instead of the 5-op reciprocal division.
hipError_t launch_selftest_div(float b, int use_fma, float c, unsigned first_bits, unsigned last_bits,
                               unsigned long long *d_mismatches, hipStream_t stream);

} // namespace canny
