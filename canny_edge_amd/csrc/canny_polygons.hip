// canny_polygons.hip -- polygon approximation of stored contour chains: for every chain of a contours call the vertices
// that Douglas-Peucker keeps at a tolerance given absolutely and / or relative to the chain's own length (the use of
// cv::approxPolyDP(c, eps * cv::arcLength(c, true), true)), with the length, twice the area and the convexity of the
// polygon, CSR-shaped over the records.  Everything is integers.  DESIGN.md section 19.
//
// The stage reads what a contours call stored (chain_offsets, points) and runs behind it on the same stream:
//
//   simplify : one wave per stored record.  A chain of at most 64 points lives one point per lane: the farthest point from
//              P_0 and every run's farthest point from its base are wave maxima over a packed key (the distance in the
//              high word, the complemented position in the low word: ties go to the smallest position), the vertex set is
//              a 64-bit mask in scalar registers.  That path touches no LDS and no flag byte; its one store besides the
//              count is the finished mask, parked for the emit kernel (8 bytes per record).  A longer chain is strided
//              by the lanes over the stored points, its vertex flags are one byte per point slot in the workspace.  The
//              recursion of the rule is a stackless left-to-right descent: the current run is (a, b); if it splits at m,
//              m is flagged and the run becomes (a, m); otherwise the run becomes (b, next flagged position after b).
//              The flags to the right of b ARE the stack.  vertex_offsets[j + 1] receives the count V.
//   scan     : vertex_offsets[1 .. R] become inclusive prefix sums in place: per block of 2048 entries, then the block
//              sums by one block, then the sums added back.  No atomics.
//   emit     : one wave per record goes over the chain 64 positions at a time; the flagged positions are ranked with a
//              ballot and a popcount and stored at vertices[vertex_offsets[j] + rank] below vertex_capacity.  The same
//              pass carries the last two and the first two vertices along and sums the shoelace terms and the signs of
//              the turns, so area2 and convex come from the vertex set, not from what fitted into the caller's buffer.
//
// R = min(offsets[n_frames], capacity) is read on the device; the grids are fixed by capacity.  Every output element is
// stored once by one wave, nothing depends on the order in which waves run: the output is the same bytes on every run.
// Every loop is bounded by the chain's length: no input can spin a kernel.
#include "canny_kernels.h"
#include "canny_wave.h"

#include <algorithm>

namespace canny {

namespace {

constexpr int kPgBlock = 256;         // 4 waves: 4 records per workgroup step
constexpr int kPgScanPerThread = 8;   // the scan: 8 consecutive entries per thread
constexpr int kPgScanChunk = 256 * kPgScanPerThread;
constexpr unsigned kPgEpsMax = 1u << 24;

// a wave-uniform 64-bit value as a scalar
__device__ __forceinline__ unsigned long long pg_uniform(unsigned long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ long long pg_cross(int ax, int ay, int bx, int by)
{
    return (long long)ax * by - (long long)ay * bx;
}

// |cross(B - A, P - A)|: the coordinates lie below 32768, so the value lies below 2^31
__device__ __forceinline__ unsigned pg_dist(int ax, int ay, int bx, int by, int px, int py)
{
    const long long c = pg_cross(bx - ax, by - ay, px - ax, py - ay);
    return (unsigned)(c < 0 ? -c : c);
}

// c^2 * 2^16 > eps^2 * |B - A|^2, exactly: c < 2^31, eps <= 2^24, |B - A|^2 < 2^31
__device__ __forceinline__ bool pg_splits(unsigned c, int dx, int dy, unsigned eps)
{
    const unsigned __int128 lhs = (unsigned __int128)((unsigned long long)c * c) << 16;
    const unsigned long long base2 = (unsigned long long)((long long)dx * dx + (long long)dy * dy);
    const unsigned __int128 rhs = (unsigned __int128)((unsigned long long)eps * eps) * base2;
    return lhs > rhs;
}

__device__ __forceinline__ unsigned pg_eps(unsigned epsilon_q8, unsigned ratio_q16, unsigned long long length_q8)
{
    const unsigned long long e = (unsigned long long)epsilon_q8 + (((unsigned long long)ratio_q16 * length_q8) >> 16);
    return e < kPgEpsMax ? (unsigned)e : kPgEpsMax;
}

// a step with both coordinates changing counts 362, one with exactly one of them changing 256, a zero step nothing
__device__ __forceinline__ void pg_step(int dx, int dy, bool &axis, bool &diag)
{
    diag = dx != 0 && dy != 0;
    axis = (dx != 0) != (dy != 0);
}

#define PG_FOR_EACH_RECORD(n_records, j)                                                                                \
    for (unsigned long long j = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6,                       \
                            stride_ = ((unsigned long long)gridDim.x * blockDim.x) >> 6;                               \
         j < (n_records); j += stride_)

// vertex_offsets[j + 1] = V of record j (0 for a cut chain), vertex_offsets[0] = 0; masks[j] = the vertex set of a chain
// of at most 64 points; flags[chain_offsets[j] + i] = position i of a longer chain is a vertex; measures[j][0 .. 1] =
// V, length_q8 ((-1, 0, 0, 0) for a cut chain).
__global__ __launch_bounds__(kPgBlock) void pg_simplify_kernel(const unsigned long long *__restrict__ offsets, int n_frames,
                                                               unsigned long long capacity,
                                                               const unsigned long long *__restrict__ chain_offsets,
                                                               const int *__restrict__ points,
                                                               unsigned long long point_capacity, int width,
                                                               unsigned epsilon_q8, unsigned ratio_q16,
                                                               unsigned long long *__restrict__ vertex_offsets,
                                                               unsigned long long *__restrict__ masks, uint8_t *flags_all,
                                                               long long *__restrict__ measures)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long total = offsets[n_frames];
    const unsigned long long n_records = total < capacity ? total : capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) vertex_offsets[0] = 0ull;
    PG_FOR_EACH_RECORD(n_records, j)
    {
        const unsigned long long begin = chain_offsets[j], end = chain_offsets[j + 1];
        if (end > point_capacity || end < begin) { // a cut chain
            if (lane == 0) {
                vertex_offsets[j + 1] = 0ull;
                if (measures) {
                    long long *m = measures + 4 * j;
                    m[0] = -1, m[1] = 0, m[2] = 0, m[3] = 0;
                }
            }
            continue;
        }
        const unsigned long long n = end - begin;
        const int *p = points + begin;
        unsigned long long n_vertices, length_q8;
        if (n <= 64) {
            // ---- one point per lane; the vertex set is a mask ----
            const int nn = (int)n;
            const bool mine = lane < nn;
            const int px = mine ? p[lane] : 0;
            const int y = px / width, x = px - y * width;
            const int nxt = lane + 1 == nn ? 0 : lane + 1;
            const int dx = __shfl(x, nxt) - x, dy = __shfl(y, nxt) - y;
            bool axis, diag;
            pg_step(dx, dy, axis, diag);
            length_q8 = 256ull * (unsigned)__popcll(__ballot(mine && axis)) + 362ull * (unsigned)__popcll(__ballot(mine && diag));
            const unsigned eps = pg_eps(epsilon_q8, ratio_q16, length_q8);
            const int x0 = __builtin_amdgcn_readfirstlane(x), y0 = __builtin_amdgcn_readfirstlane(y);
            const unsigned low = 63u - (unsigned)lane; // the complemented position
            const unsigned d0 = (unsigned)((x - x0) * (x - x0) + (y - y0) * (y - y0));
            unsigned long long key = pg_uniform(wave_max(mine ? ((unsigned long long)d0 << 32) | low : 0ull));
            int a = 0, b = 63 - (int)(key & 63u); // b = k
            unsigned long long mask = nn ? 1ull | (1ull << b) : 0ull;
            for (int guard = 0; guard < 2 * nn + 2 && nn >= 2; guard++) {
                if (b - a >= 2) {
                    const int bl = b == nn ? 0 : b;
                    const int ax = __builtin_amdgcn_readlane(x, a), ay = __builtin_amdgcn_readlane(y, a);
                    const int bx = __builtin_amdgcn_readlane(x, bl), by = __builtin_amdgcn_readlane(y, bl);
                    const bool in = lane > a && lane < b;
                    const unsigned c = pg_dist(ax, ay, bx, by, x, y);
                    key = pg_uniform(wave_max(in ? ((unsigned long long)c << 32) | low : 0ull));
                    if (pg_splits((unsigned)(key >> 32), bx - ax, by - ay, eps)) {
                        b = 63 - (int)(key & 63u);
                        mask |= 1ull << b;
                        continue;
                    }
                }
                a = b;
                if (a >= nn) break;
                const unsigned long long rest = a + 1 < 64 ? mask >> (a + 1) : 0ull;
                b = rest ? a + 1 + (int)__builtin_ctzll(rest) : nn;
            }
            n_vertices = (unsigned)__popcll(mask);
            if (lane == 0) masks[j] = mask;
        } else {
            // ---- the lanes stride over the stored points; the vertex set is a byte per point slot ----
            uint8_t *flags = flags_all + begin;
            unsigned n_axis = 0, n_diag = 0;
            const int p0 = p[0];
            const int y0 = p0 / width, x0 = p0 - y0 * width;
            unsigned long long key = 0;
            for (unsigned long long i = lane; i < n; i += 64) {
                const int pi = p[i], pn = p[i + 1 == n ? 0 : i + 1];
                const int yi = pi / width, xi = pi - yi * width, yn = pn / width, xn = pn - yn * width;
                bool axis, diag;
                pg_step(xn - xi, yn - yi, axis, diag);
                n_axis += axis, n_diag += diag;
                const unsigned d0 = (unsigned)((xi - x0) * (xi - x0) + (yi - y0) * (yi - y0));
                const unsigned long long k = ((unsigned long long)d0 << 32) | (0xFFFFFFFFu - (unsigned)i);
                key = k > key ? k : key;
                flags[i] = 0;
            }
            length_q8 = 256ull * wave_sum<unsigned long long>(n_axis) + 362ull * wave_sum<unsigned long long>(n_diag);
            const unsigned eps = pg_eps(epsilon_q8, ratio_q16, length_q8);
            key = pg_uniform(wave_max(key));
            unsigned long long a = 0, b = 0xFFFFFFFFu - (unsigned)key; // b = k
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (lane == 0) flags[0] = 1, flags[b] = 1;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            n_vertices = b ? 2 : 1;
            for (unsigned long long guard = 0; guard < 2 * n + 2; guard++) {
                if (b - a >= 2) {
                    const int pa = p[a], pb = p[b == n ? 0 : b];
                    const int ay = pa / width, ax = pa - ay * width, by = pb / width, bx = pb - by * width;
                    key = 0;
                    // four loads in flight per lane: a long run is bound by the latency of its loads
                    for (unsigned long long i = a + 1 + lane; i < b; i += 256) {
                        int pi[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) pi[u] = i + 64 * u < b ? p[i + 64 * u] : 0;
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            if (i + 64 * u >= b) break;
                            const int yi = pi[u] / width, xi = pi[u] - yi * width;
                            const unsigned c = pg_dist(ax, ay, bx, by, xi, yi);
                            const unsigned long long k =
                                ((unsigned long long)c << 32) | (0xFFFFFFFFu - (unsigned)(i + 64 * u));
                            key = k > key ? k : key;
                        }
                    }
                    key = pg_uniform(wave_max(key));
                    if (pg_splits((unsigned)(key >> 32), bx - ax, by - ay, eps)) {
                        b = 0xFFFFFFFFu - (unsigned)key;
                        if (lane == 0) flags[b] = 1;
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        n_vertices++;
                        continue;
                    }
                }
                a = b;
                if (a >= n) break;
                b = n;
                for (unsigned long long i0 = a + 1; i0 < n; i0 += 64) {
                    const unsigned long long i = i0 + lane;
                    const unsigned long long set = __ballot(i < n && ((volatile uint8_t *)flags)[i] != 0);
                    if (set) {
                        b = i0 + (unsigned)__builtin_ctzll(set);
                        break;
                    }
                }
            }
        }
        if (lane == 0) {
            vertex_offsets[j + 1] = n_vertices;
            if (measures) measures[4 * j] = (long long)n_vertices, measures[4 * j + 1] = (long long)length_q8;
        }
    }
}

__device__ __forceinline__ unsigned long long pg_records(const unsigned long long *offsets, int n_frames,
                                                         unsigned long long capacity)
{
    const unsigned long long total = offsets[n_frames];
    return total < capacity ? total : capacity;
}

// entries 1 + 2048 * block ... of vertex_offsets, up to entry R: inclusive prefix sums within the block's chunk, in place;
// block_sums[block] = the chunk's sum
__global__ __launch_bounds__(256) void pg_scan_chunks_kernel(const unsigned long long *__restrict__ offsets, int n_frames,
                                                             unsigned long long capacity,
                                                             unsigned long long *__restrict__ vertex_offsets,
                                                             unsigned long long *__restrict__ block_sums)
{
    __shared__ unsigned long long s_wave[4];
    const unsigned long long n_records = pg_records(offsets, n_frames, capacity);
    const unsigned long long first = 1ull + (unsigned long long)blockIdx.x * kPgScanChunk + threadIdx.x * kPgScanPerThread;
    unsigned long long v[kPgScanPerThread], sum = 0;
#pragma unroll
    for (int k = 0; k < kPgScanPerThread; k++) {
        v[k] = first + k <= n_records ? vertex_offsets[first + k] : 0ull;
        sum += v[k];
    }
    unsigned long long chunk;
    unsigned long long run = block_exclusive_scan(sum, s_wave, &chunk);
#pragma unroll
    for (int k = 0; k < kPgScanPerThread; k++) {
        run += v[k];
        if (first + k <= n_records) vertex_offsets[first + k] = run;
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = chunk;
}

// block_sums[b] -> the sum of the chunks before b
__global__ __launch_bounds__(256) void pg_scan_sums_kernel(unsigned long long *__restrict__ block_sums, unsigned n_blocks)
{
    __shared__ unsigned long long s_wave[4];
    unsigned long long carry = 0;
    for (unsigned base = 0; base < n_blocks; base += 256) {
        const unsigned i = base + threadIdx.x;
        unsigned long long chunk;
        const unsigned long long ex = block_exclusive_scan(i < n_blocks ? block_sums[i] : 0ull, s_wave, &chunk);
        if (i < n_blocks) block_sums[i] = carry + ex;
        carry += chunk;
    }
}

__global__ __launch_bounds__(256) void pg_scan_add_kernel(const unsigned long long *__restrict__ offsets, int n_frames,
                                                          unsigned long long capacity,
                                                          unsigned long long *__restrict__ vertex_offsets,
                                                          const unsigned long long *__restrict__ block_sums)
{
    const unsigned long long n_records = pg_records(offsets, n_frames, capacity);
    const unsigned long long before = block_sums[blockIdx.x];
    if (!before) return;
    const unsigned long long first = 1ull + (unsigned long long)blockIdx.x * kPgScanChunk + threadIdx.x * kPgScanPerThread;
#pragma unroll
    for (int k = 0; k < kPgScanPerThread; k++)
        if (first + k <= n_records) vertex_offsets[first + k] += before;
}

// vertices[vertex_offsets[j] + rank] = the pixel of the rank-th vertex of record j, below vertex_capacity;
// measures[j][2 .. 3] = area2, convex.  vertex_offsets is scanned; masks / flags are as the simplify kernel left them.
__global__ __launch_bounds__(kPgBlock) void pg_emit_kernel(const unsigned long long *__restrict__ offsets, int n_frames,
                                                           unsigned long long capacity,
                                                           const unsigned long long *__restrict__ chain_offsets,
                                                           const int *__restrict__ points,
                                                           unsigned long long point_capacity, int width,
                                                           const unsigned long long *__restrict__ vertex_offsets,
                                                           const unsigned long long *__restrict__ masks,
                                                           const uint8_t *__restrict__ flags_all, int *__restrict__ vertices,
                                                           unsigned long long vertex_capacity,
                                                           long long *__restrict__ measures)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long n_records = pg_records(offsets, n_frames, capacity);
    const unsigned long long lower = (1ull << lane) - 1ull;
    PG_FOR_EACH_RECORD(n_records, j)
    {
        const unsigned long long begin = chain_offsets[j], end = chain_offsets[j + 1];
        if (end > point_capacity || end < begin) continue; // a cut chain: the simplify kernel wrote its measures
        const unsigned long long n = end - begin;
        const unsigned long long out_at = vertex_offsets[j];
        if (!measures && out_at >= vertex_capacity) continue;
        const int *p = points + begin;
        const uint8_t *flags = flags_all + begin;
        const unsigned long long mask = n <= 64 ? masks[j] : 0ull;
        unsigned long long have = 0; // vertices before this round
        int l1x = 0, l1y = 0, l2x = 0, l2y = 0; // the last and the last but one vertex so far
        int f0x = 0, f0y = 0, f1x = 0, f1y = 0; // the first two
        long long area = 0;
        bool pos = false, neg = false;
        for (unsigned long long i0 = 0; i0 < n; i0 += 64) {
            const unsigned long long i = i0 + lane;
            const bool flag = i < n && (n <= 64 ? (mask >> lane) & 1ull : flags[i] != 0);
            const unsigned long long set = __ballot(flag);
            if (!set) continue;
            const int px = flag ? p[i] : 0;
            const int y = px / width, x = px - y * width;
            const unsigned long long below = set & lower;
            const unsigned n_below = (unsigned)__popcll(below);
            const unsigned long long rank = have + n_below;
            if (flag && vertices && out_at + rank < vertex_capacity) vertices[out_at + rank] = px;
            // the two vertices before this lane's: in this round, or carried
            const int s1 = below ? 63 - (int)__builtin_clzll(below) : 0;
            const unsigned long long below2 = below & ((1ull << s1) - 1ull);
            const int s2 = below2 ? 63 - (int)__builtin_clzll(below2) : 0;
            int q1x = __shfl(x, s1), q1y = __shfl(y, s1), q2x = __shfl(x, s2), q2y = __shfl(y, s2);
            if (n_below == 0) q1x = l1x, q1y = l1y, q2x = l2x, q2y = l2y;
            else if (n_below == 1) q2x = l1x, q2y = l1y;
            long long turn = 0;
            if (flag && rank >= 1) area += pg_cross(q1x, q1y, x, y);
            if (flag && rank >= 2) turn = pg_cross(q1x - q2x, q1y - q2y, x - q1x, y - q1y);
            pos |= __ballot(turn > 0) != 0ull;
            neg |= __ballot(turn < 0) != 0ull;
            const unsigned n_set = (unsigned)__popcll(set);
            const int a0 = (int)__builtin_ctzll(set);
            const unsigned long long set1 = set & (set - 1ull);
            const int a1 = set1 ? (int)__builtin_ctzll(set1) : 0;
            if (have == 0) {
                f0x = __shfl(x, a0), f0y = __shfl(y, a0);
                if (n_set >= 2) f1x = __shfl(x, a1), f1y = __shfl(y, a1);
            } else if (have == 1) {
                f1x = __shfl(x, a0), f1y = __shfl(y, a0);
            }
            const int z1 = 63 - (int)__builtin_clzll(set);
            const unsigned long long setz = set & ~(1ull << z1);
            if (setz) {
                const int z2 = 63 - (int)__builtin_clzll(setz);
                l2x = __shfl(x, z2), l2y = __shfl(y, z2);
            } else {
                l2x = l1x, l2y = l1y;
            }
            l1x = __shfl(x, z1), l1y = __shfl(y, z1);
            have += n_set;
        }
        if (!measures) continue;
        long long area2 = (long long)wave_sum((unsigned long long)area);
        if (have >= 1) area2 += pg_cross(l1x, l1y, f0x, f0y);
        if (have >= 3) {
            const long long t1 = pg_cross(l1x - l2x, l1y - l2y, f0x - l1x, f0y - l1y);
            const long long t2 = pg_cross(f0x - l1x, f0y - l1y, f1x - f0x, f1y - f0y);
            pos |= t1 > 0 || t2 > 0;
            neg |= t1 < 0 || t2 < 0;
        }
        if (lane == 0) {
            measures[4 * j + 2] = area2 < 0 ? -area2 : area2;
            measures[4 * j + 3] = have >= 3 && pos != neg ? 1 : 0;
        }
    }
}

} // namespace

LaunchPlan plan_pg_records(unsigned long long capacity) { return capped_plan(capacity, kPgBlock / 64, 1u << 16); }
LaunchPlan plan_pg_scan_sums(unsigned long long capacity)
{
    return capped_plan(polygons_scan_blocks(capacity), 256, 1);
}

unsigned long long polygons_scan_blocks(unsigned long long capacity)
{
    return std::max<unsigned long long>(1, (capacity + kPgScanChunk - 1) / kPgScanChunk);
}

hipError_t launch_pg_simplify(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                              const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity,
                              int width, unsigned epsilon_q8, unsigned ratio_q16, unsigned long long *vertex_offsets,
                              unsigned long long *masks, uint8_t *flags, long long *measures, hipStream_t stream)
{
    hipLaunchKernelGGL(pg_simplify_kernel, dim3(plan_pg_records(capacity).grid), dim3(kPgBlock), 0, stream, offsets,
                       n_frames, capacity, chain_offsets, points, point_capacity, width, epsilon_q8, ratio_q16,
                       vertex_offsets, masks, flags, measures);
    return hipGetLastError();
}

hipError_t launch_pg_scan(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                          unsigned long long *vertex_offsets, unsigned long long *block_sums, hipStream_t stream)
{
    const unsigned n_blocks = (unsigned)polygons_scan_blocks(capacity);
    hipLaunchKernelGGL(pg_scan_chunks_kernel, dim3(n_blocks), dim3(256), 0, stream, offsets, n_frames, capacity,
                       vertex_offsets, block_sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_blocks == 1) return e;
    hipLaunchKernelGGL(pg_scan_sums_kernel, dim3(plan_pg_scan_sums(capacity).grid), dim3(256), 0, stream, block_sums,
                       n_blocks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(pg_scan_add_kernel, dim3(n_blocks), dim3(256), 0, stream, offsets, n_frames, capacity, vertex_offsets,
                       (const unsigned long long *)block_sums);
    return hipGetLastError();
}

hipError_t launch_pg_emit(const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                          const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity,
                          int width, const unsigned long long *vertex_offsets, const unsigned long long *masks,
                          const uint8_t *flags, int *vertices, unsigned long long vertex_capacity, long long *measures,
                          hipStream_t stream)
{
    hipLaunchKernelGGL(pg_emit_kernel, dim3(plan_pg_records(capacity).grid), dim3(kPgBlock), 0, stream, offsets,
                       n_frames, capacity, chain_offsets, points, point_capacity, width, vertex_offsets, masks, flags,
                       vertices, vertex_capacity, measures);
    return hipGetLastError();
}

} // namespace canny
