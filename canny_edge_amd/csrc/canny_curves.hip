// canny_curves.hip -- edge curves of a finished edge map, per frame of a batch: edge linking.  Every edge pixel is taken
// once, in order along its curve; curves are split at junctions; open and closed curves are told apart.  The output has the
// two-level CSR shape of the contour chains.  The rule: include/canny_hip.h; DESIGN.md section 28.
//
//   count : one wave per image row (grid-stride over the rows of the batch), the row in chunks of 64 columns, one lane per
//           pixel.  The chunk's nodes (deg != 2) and closed-curve candidates (path pixels without a link in directions
//           4 .. 7) are found word-parallel from the three row words: links per direction as shifted ANDs, the degree as a
//           bit-sliced count.  The row words are loaded 64 chunks at a time, one chunk per lane, and a ballot names the
//           chunks that hold a pixel; a chunk without a node or candidate is passed over.  A node lane walks each of its <= 4 links to the
//           node at the other end and owns the curve if its key is the smaller one; a candidate lane walks from its
//           smaller direction, gives up at the first node or smaller index and owns the closed curve if it comes back to
//           itself.  Per row the kept curves and their points are summed over the wave; launch_points_scan (twice) turns
//           the row sums into row bases, offsets[] and point_offsets[].
//   write : the same walks again, the lengths of the <= 4 owned curves kept in registers; two wave prefix sums onto the
//           row bases give every curve its record number and the position of its first point, in key order (raster order
//           of the start, then first direction).  The owner stores chain_offsets[record + 1] and the record, then walks the
//           curve once more and stores its points below point_capacity.
//
// No counter hands out space, no atomic, nothing depends on the order in which waves run: the output is the same bytes on
// every run.  The walking window is the contours' (canny_bit_walk.h).  Every walk is capped at height * width steps: an
// open walk visits a path pixel at most once and a closed one never passes its start, so no map reaches the cap, and no
// input can spin a kernel.
#include "canny_bit_walk.h"
#include "canny_kernels.h"

#include "canny_hip.h"

namespace canny {

namespace {

constexpr int kCvBlock = 256; // 4 waves: 4 image rows per workgroup step

// the links of a set pixel from its ring (bit d = the neighbour in direction d is set): 4-neighbours always, a diagonal
// only if neither of the two pixels 4-adjacent to both is set
__device__ __forceinline__ unsigned cv_links(unsigned r)
{
    const unsigned rl = ((r << 1) | (r >> 7)) & 0xFFu, rr = ((r >> 1) | (r << 7)) & 0xFFu;
    return r & (0x55u | ~(rl | rr)) & 0xFFu;
}

// what a chunk's lanes have to do: bit i = column 64 * k + i
struct CvChunk {
    uint64_t nodes;      // deg != 2
    uint64_t candidates; // deg == 2 and no link in directions 4 .. 7
};

// three consecutive words of one row: columns 64 * (k - 1) .. 64 * (k + 2) - 1
struct CvRow3 {
    uint64_t w, c, e;
    __device__ __forceinline__ uint64_t west() const { return (c << 1) | (w >> 63); } // bit i = column 64 * k + i - 1
    __device__ __forceinline__ uint64_t east() const { return (c >> 1) | (e << 63); } // bit i = column 64 * k + i + 1
};

// word-parallel over columns 64 * k .. 64 * k + 63 of a row (mid.c != 0), from the words of the rows above and below
// (wave-uniform: every lane computes the same words)
__device__ __forceinline__ CvChunk cv_chunk(const CvRow3 &up, const CvRow3 &mid, const CvRow3 &dn)
{
    const uint64_t m = mid.c;
    const uint64_t n_e = mid.east(), n_w = mid.west(), n_n = up.c, n_s = dn.c;
    const uint64_t l[8] = {m & n_e,
                           m & dn.east() & ~(n_e | n_s),
                           m & n_s,
                           m & dn.west() & ~(n_s | n_w),
                           m & n_w,
                           m & up.west() & ~(n_w | n_n),
                           m & n_n,
                           m & up.east() & ~(n_n | n_e)};
    uint64_t ones = 0, twos = 0, fours = 0; // the degree, bit-sliced; it is at most 4
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t c1 = ones & l[i];
        ones ^= l[i];
        const uint64_t c2 = twos & c1;
        twos ^= c1;
        fours |= c2;
    }
    const uint64_t deg2 = twos & ~ones & ~fours;
    return CvChunk{m & ~deg2, m & deg2 & ~(l[4] | l[5] | l[6] | l[7])};
}

struct CvEnd {
    unsigned len; // points of the curve; 0: not a curve of this walk's (a candidate that gave up, or the cap)
    int end;      // the last listed pixel
    int last;     // the direction of the step that reached it
    bool junction; // an open walk's end has deg >= 3
};

// The walk of the rule from pixel p0 (the window w is loaded there) along its link d.  Open (closed = false): to the first
// node.  Closed candidate: until it is back at p0; it gives up at the first node or smaller index.
template <bool BITS>
__device__ __forceinline__ CvEnd cv_follow(CtWalk w, const void *__restrict__ src, const HystGeom &g, int row_bytes, int f,
                                           int p0, int d, bool closed, unsigned cap)
{
    CvEnd e{0u, p0, d, false};
    int cur = p0;
    unsigned n = 1;
    for (unsigned step = 0; step < cap; step++) {
        ct_move<BITS>(w, d, src, g, row_bytes, f);
        cur += ct_dy(d) * g.width + ct_dx(d);
        if (closed && cur == p0) {
            e.len = n;
            return e;
        }
        const unsigned l = cv_links(ct_ring(w));
        const bool node = __popc(l) != 2;
        if (closed && (node || cur < p0)) return e;
        n++, e.end = cur, e.last = d;
        if (node) {
            e.len = n, e.junction = __popc(l) >= 3;
            return e;
        }
        d = (int)__builtin_ctz((l & ~(1u << ((d + 4) & 7))) | 0x100u); // a path pixel: the link it was entered by, and one more
    }
    return e; // cannot happen
}

// The first n_store >= 1 points of the curve from p0 along d, stored at out: the walk above without its tests -- every
// pixel it leaves after the first is a path pixel of a curve whose length is known.
template <bool BITS>
__device__ __forceinline__ void cv_store(CtWalk w, const void *__restrict__ src, const HystGeom &g, int row_bytes, int f,
                                         int p0, int d, unsigned n_store, int *__restrict__ out)
{
    int cur = p0;
    out[0] = p0;
    for (unsigned i = 1; i < n_store; i++) {
        if (i > 1) d = (int)__builtin_ctz((cv_links(ct_ring(w)) & ~(1u << ((d + 4) & 7))) | 0x100u);
        ct_move<BITS>(w, d, src, g, row_bytes, f);
        cur += ct_dy(d) * g.width + ct_dx(d);
        out[i] = cur;
    }
}

// four words in four registers, indexed by selects (an indexed array would live in scratch)
struct CvSlots {
    unsigned a, b, c, d;
    __device__ __forceinline__ void set(int j, unsigned v)
    {
        a = j == 0 ? v : a, b = j == 1 ? v : b, c = j == 2 ? v : c, d = j == 3 ? v : d;
    }
    __device__ __forceinline__ unsigned get(int j) const { return j == 0 ? a : j == 1 ? b : j == 2 ? c : d; }
};

// The kept curves that the lane's pixel (y, x) owns, in key order: their number; len / end / meta (first direction, last
// direction << 4, flags << 8) per curve in the slots; *pts receives the sum of the lengths.
template <bool BITS>
__device__ __forceinline__ unsigned cv_owned(const CtWalk &w0, bool is_node, const void *__restrict__ src,
                                             const HystGeom &g, int row_bytes, int f, int p0, int min_length, unsigned cap,
                                             CvSlots &len, CvSlots &end, CvSlots &meta, unsigned *pts)
{
    const unsigned l = cv_links(ct_ring(w0));
    unsigned n = 0, sum = 0;
    if (!l) { // an isolated pixel
        if (min_length <= 1) {
            len.set(0, 1u), end.set(0, (unsigned)p0), meta.set(0, (unsigned)CANNY_HIP_CURVE_ISOLATED << 8);
            n = 1, sum = 1;
        }
    } else if (is_node) {
        const unsigned start_flag = __popc(l) >= 3 ? (unsigned)CANNY_HIP_CURVE_START_JUNCTION : 0u;
        for (unsigned rest = l; rest; rest &= rest - 1) {
            const int d = (int)__builtin_ctz(rest);
            const CvEnd e = cv_follow<BITS>(w0, src, g, row_bytes, f, p0, d, false, cap);
            // the curve belongs to the end with the smaller key
            if (!e.len || 8u * (unsigned)p0 + (unsigned)d > 8u * (unsigned)e.end + (unsigned)((e.last + 4) & 7)) continue;
            if ((long long)e.len < (long long)min_length) continue;
            len.set((int)n, e.len), end.set((int)n, (unsigned)e.end);
            meta.set((int)n, (unsigned)d | ((unsigned)e.last << 4) |
                                 ((start_flag | (e.junction ? (unsigned)CANNY_HIP_CURVE_END_JUNCTION : 0u)) << 8));
            n++, sum += e.len;
        }
    } else { // a closed-curve candidate
        const int d = (int)__builtin_ctz(l);
        const CvEnd e = cv_follow<BITS>(w0, src, g, row_bytes, f, p0, d, true, cap);
        if (e.len && (long long)e.len >= (long long)min_length) {
            len.set(0, e.len), end.set(0, (unsigned)e.end);
            meta.set(0, (unsigned)d | ((unsigned)e.last << 4) | ((unsigned)CANNY_HIP_CURVE_CLOSED << 8));
            n = 1, sum = e.len;
        }
    }
    *pts = sum;
    return n;
}

// WRITE = false, the count: row_curves[r] / row_points[r] = the kept curves that start in row r / their points.
// WRITE = true: row_curves / row_points as launch_points_scan leaves them (the frame's curves / points before the row),
//   offsets / point_offsets the two CSRs; chain_offsets[record + 1], records and points are stored for records below
//   capacity, points below point_capacity; chain_offsets[0] = 0.  records and points may be null.
template <bool BITS, bool WRITE>
__global__ __launch_bounds__(kCvBlock) void cv_walk_kernel(const void *__restrict__ src, HystGeom g, int row_bytes,
                                                           int min_length, uint32_t *__restrict__ row_curves,
                                                           uint32_t *__restrict__ row_points,
                                                           const unsigned long long *__restrict__ offsets,
                                                           const unsigned long long *__restrict__ point_offsets,
                                                           unsigned long long *__restrict__ chain_offsets,
                                                           unsigned long long capacity, int *__restrict__ records,
                                                           int *__restrict__ points, unsigned long long point_capacity)
{
    const int lane = threadIdx.x & 63;
    const unsigned cap = (unsigned)(g.height * g.width);
    CT_FOR_EACH_ROW(g, r)
    {
        // the row is the wave's: say so, and the row words and bases are loaded once per wave
        const int f = __builtin_amdgcn_readfirstlane((int)(r / (size_t)g.height));
        const int y = __builtin_amdgcn_readfirstlane((int)(r - (size_t)f * g.height));
        unsigned run = 0, run_pts = 0; // WRITE: the row's curves / points before this chunk; count: the lane's sums
        unsigned long long rec_base = 0, pt_base = 0;
        if constexpr (WRITE) {
            rec_base = offsets[f] + row_curves[r];
            pt_base = point_offsets[f] + row_points[r];
        }
        // 64 chunks at a time: lane i loads the words of chunk k0 + i (one load per row instead of one per chunk and row),
        // a ballot names the chunks that hold a pixel, and only those are looked at, their words taken from the lanes
        for (int k0 = 0; k0 < g.tiles_x; k0 += 64)
        for (uint64_t mid_l = ct_word<BITS>(src, g, row_bytes, f, y, k0 + lane), busy = __ballot(mid_l != 0ull),
                      up_l = busy ? ct_word<BITS>(src, g, row_bytes, f, y - 1, k0 + lane) : 0ull,
                      dn_l = busy ? ct_word<BITS>(src, g, row_bytes, f, y + 1, k0 + lane) : 0ull;
             busy; busy &= busy - 1) {
            const int j = (int)__builtin_ctzll(busy), k = k0 + j; // wave-uniform
            // word jj of the group from its lane; the two words beside the group (rows wider than 4096 pixels) from memory
            auto row3 = [&](uint64_t v_l, int yy) {
                return CvRow3{j > 0 ? __shfl(v_l, j - 1) : ct_word<BITS>(src, g, row_bytes, f, yy, k - 1), __shfl(v_l, j),
                              j < 63 ? __shfl(v_l, j + 1) : ct_word<BITS>(src, g, row_bytes, f, yy, k + 1)};
            };
            const CvChunk ch = cv_chunk(row3(up_l, y - 1), row3(mid_l, y), row3(dn_l, y + 1));
            if (!(ch.nodes | ch.candidates)) continue; // wave-uniform
            const bool is_node = (ch.nodes >> lane) & 1ull, mine = ((ch.nodes | ch.candidates) >> lane) & 1ull;
            const int x = (k << 6) + lane, p0 = y * g.width + x;
            CvSlots len{0, 0, 0, 0}, end{0, 0, 0, 0}, meta{0, 0, 0, 0};
            CtWalk w0;
            unsigned n = 0, pts = 0;
            if (mine) {
                w0.y = y, w0.x = x;
                ct_load<BITS>(w0, src, g, row_bytes, f);
                n = cv_owned<BITS>(w0, is_node, src, g, row_bytes, f, p0, min_length, cap, len, end, meta, &pts);
            }
            if constexpr (!WRITE) {
                run += n, run_pts += pts;
            } else {
                unsigned incl = n, incl_pts = pts;
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {
                    const unsigned t = __shfl_up(incl, s), tp = __shfl_up(incl_pts, s);
                    if (lane >= s) incl += t, incl_pts += tp;
                }
                unsigned long long at = rec_base + run + (incl - n);          // the record of the lane's first curve
                unsigned long long begin = pt_base + run_pts + (incl_pts - pts); // ... and where its points start
                run += __shfl(incl, 63), run_pts += __shfl(incl_pts, 63);
                for (unsigned q = 0; q < n; q++, at++) {
                    const unsigned ln = len.get((int)q), mt = meta.get((int)q);
                    const unsigned long long first = begin;
                    begin += ln;
                    if (at >= capacity) break;
                    chain_offsets[at + 1] = begin;
                    if (records) {
                        int *rec = records + at * CANNY_HIP_CURVE_RECORD;
                        rec[CANNY_HIP_CURVE_START] = p0, rec[CANNY_HIP_CURVE_END] = (int)end.get((int)q);
                        rec[CANNY_HIP_CURVE_POINTS] = (int)ln;
                        rec[CANNY_HIP_CURVE_FLAGS] = (int)((mt >> 8) | ((mt & 7u) << CANNY_HIP_CURVE_FIRST_DIR_SHIFT) |
                                                           (((mt >> 4) & 7u) << CANNY_HIP_CURVE_LAST_DIR_SHIFT));
                    }
                    if (points && first < point_capacity) {
                        const unsigned long long room = point_capacity - first;
                        cv_store<BITS>(w0, src, g, row_bytes, f, p0, (int)(mt & 7u), room < ln ? (unsigned)room : ln,
                                       points + first);
                    }
                }
            }
        }
        if constexpr (!WRITE) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) run += __shfl_xor(run, s), run_pts += __shfl_xor(run_pts, s);
            if (lane == 0) row_curves[r] = run, row_points[r] = run_pts;
        } else {
            if (r == 0 && lane == 0) chain_offsets[0] = 0ull;
        }
    }
}

#define CV_LAUNCH(WRITE, ...)                                                                                           \
    do {                                                                                                                \
        const unsigned grid_ = plan_cv_rows(g).grid;                                                                    \
        if (bits)                                                                                                       \
            hipLaunchKernelGGL((cv_walk_kernel<true, WRITE>), dim3(grid_), dim3(kCvBlock), 0, stream,                   \
                               (const void *)bits, g, (g.width + 7) / 8, __VA_ARGS__);                                  \
        else                                                                                                            \
            hipLaunchKernelGGL((cv_walk_kernel<false, WRITE>), dim3(grid_), dim3(kCvBlock), 0, stream,                  \
                               (const void *)strong, g, (g.width + 7) / 8, __VA_ARGS__);                                \
        return hipGetLastError();                                                                                       \
    } while (0)

} // namespace

LaunchPlan plan_cv_rows(const HystGeom &g)
{
    return capped_plan((unsigned long long)g.n_frames * g.height, kCvBlock / 64, 1u << 16);
}

hipError_t launch_cv_count(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_length,
                           uint32_t *row_curves, uint32_t *row_points, hipStream_t stream)
{
    CV_LAUNCH(false, min_length, row_curves, row_points, (const unsigned long long *)nullptr,
              (const unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (int *)nullptr, (int *)nullptr, 0ull);
}

hipError_t launch_cv_write(const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_length,
                           uint32_t *row_curves, uint32_t *row_points, const unsigned long long *offsets,
                           const unsigned long long *point_offsets, unsigned long long *chain_offsets,
                           unsigned long long capacity, int *records, int *points, unsigned long long point_capacity,
                           hipStream_t stream)
{
    if (!points) point_capacity = 0;
    CV_LAUNCH(true, min_length, row_curves, row_points, offsets, point_offsets, chain_offsets, capacity, records, points,
              point_capacity);
}

} // namespace canny
