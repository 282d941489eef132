// canny_thin.hip -- thinning of packed bit maps to one-pixel skeletons (Zhang-Suen, Guo-Hall).  The rule is part of the
// interface (include/canny_hip.h); tests/thin_rule.py restates it in numpy, canny_thin_host.cpp pixel by
// pixel in plain C++.  All bit operations; every output byte has one writer; the only atomics are integer sums (the deletions
// of a frame and iteration, the set bits of an output frame): the same bytes on every run.
//
//   One kernel serves both routes: a workgroup of 256 lanes per tile of 8 words x 64 rows (512 x 64 pixels) and trip of a
//   capped grid runs n_sub sub-iterations on the tile without leaving LDS.
//   stage     : the tile's words plus n_sub rows above and below and one word left and right go to LDS as LSB-first 64-bit
//               words (the morphology's morph_load); the outside-of-frame zero is put in HERE: no lane tests a pixel.
//   sub-iter  : every staged word from the word, its two row neighbours and the three words of the rows above and below: the
//               eight neighbour words are funnel shifts by one, the counts of the rule are bit-sliced "exactly one / at least
//               two" pairs (two |= one & t; one ^= t), 64 pixels at once.  Two LDS arrays, ping-pong, a barrier a sub-iteration.
//               What lies beyond the staged region reads 0, so after j sub-iterations the staged words are exact except for a
//               fringe of j pixels at the staged border; where that border is the frame border the zero is exact.  n_sub rows
//               and 64 >= n_sub columns of halo keep the fringe out of the tile.
//   stepwise  : n_sub = 1, one launch per sub-iteration, through global memory: the cross-check.
//   fused     : n_sub = 2 F for F full iterations; a tile stops when a full iteration deleted nothing in its whole staged
//               region (the state is then a fixed point of that region).
//   deleted   : per frame and iteration the deletions of the tiles' own pixels, one atomic add per wave that deleted something.
//               A workgroup that arrives at a frame whose preceding iteration (final by stream order) deleted nothing copies
//               the tile from source to destination and does nothing else: the frame is at its fixed point.
//   The iterations of a call run in chunks of 8, 16, then 32: the words of a chunk live in one half of a ring of two, a
//   one-thread-per-frame kernel folds them into the frame's state behind the chunk, and max_iterations = 0 reads ONE device
//   word behind that: the frames that have not yet reported an iteration without deletions.
#include "canny_bit_words.h" // flip_bits, morph_load, funnel, store_word
#include "canny_kernels.h"
#include "canny_thin_words.h" // OneTwo, thin_deletions

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 8, kTH = 64;       // output tile: words (of 64 columns) x rows
constexpr int kMaxFuse = 8;            // "thin_fuse"
constexpr int kMaxSub = 2 * kMaxFuse;  // sub-iterations of a launch = its halo rows
constexpr int kSW = kTW + 2;           // staged words of a row: one to the left, one to the right
constexpr int kSH = kTH + 2 * kMaxSub; // staged rows at most
constexpr unsigned kGridCap = 4096;
constexpr int kChunk = 32;             // iterations of a chunk at most: the words of a frame in one half of the ring
// Which fuse automatic takes (0: the stepwise route).  Measured on the MI355X at 128 x 4K (DESIGN.md section 37,
// profiles/thin.jsonl): the fastest call to the fixed point on strokes 8 thick is fused at 4 (3.20 ms; 2: 3.26, 8: 3.33,
// stepwise 5.71); with max_iterations given, 2 is 4 % faster than 4.
constexpr int kAutoFuse = 4;
constexpr int kFusedDefault = 4; // the fuse of "thin_route" 2 with "thin_fuse" 0 if kAutoFuse is 0

struct ThinArgs {
    const void *src;
    uint8_t *dst;
    unsigned long long *del_cur;        // [n_frames][kChunk]: the deletions of the iterations chunk_i0 .. of this chunk
    const unsigned long long *del_prev; // the half of the preceding chunk; its last iteration sits at prev_off
    unsigned long long *state;          // [n_frames][4], or null: the launch that writes the caller's output counts its bits
    HystGeom g;                         // tiles_x = the words of a row
    int rb;                             // bytes of a packed row
    unsigned long long n_units;
    unsigned trips, tiles_x, tiles_y;   // tiles of this kernel, not of g
    int src_plane, vec_src, vec_dst;
    int sub0, n_sub;                    // the first sub-iteration's parity, the sub-iterations of the launch (1 .. kMaxSub)
    unsigned i0, chunk_i0;              // the iteration the launch starts in, the first iteration of its chunk
    int prev_off;
};

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int o = 32; o; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

template <int METHOD>
__global__ __launch_bounds__(kBlock) void thin_kernel(ThinArgs a)
{
    __shared__ uint64_t s_a[kSH * kSW], s_b[kSH * kSW];
    const int halo = a.n_sub;
    const unsigned per_frame = a.tiles_x * a.tiles_y;
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const unsigned f = (unsigned)(u / per_frame), t = (unsigned)(u % per_frame);
        const int k0 = (int)(t % a.tiles_x) * kTW, y0 = (int)(t / a.tiles_x) * kTH;
        const int th = min(kTH, a.g.height - y0), sh = th + 2 * halo;
        // the frame's preceding iteration, final by stream order: nothing deleted means the frame is at its fixed point
        bool skip = false;
        if (a.i0 > a.chunk_i0)
            skip = a.del_cur[(size_t)f * kChunk + (a.i0 - 1 - a.chunk_i0)] == 0;
        else if (a.i0 > 0)
            skip = a.del_prev[(size_t)f * kChunk + a.prev_off] == 0;
        unsigned set = 0; // this lane's set bits of what it stores
        if (skip) {       // the same on every lane: copy, so that the ping-pong stays consistent
            for (int i = threadIdx.x; i < th * kTW; i += kBlock) {
                const int oy = i / kTW, ox = i - oy * kTW;
                const int y = y0 + oy, k = k0 + ox;
                if (k >= a.g.tiles_x) continue;
                const uint64_t v = morph_load(a.src, a.src_plane, a.vec_src, a.g, a.rb, (int)f, y, k, 0ull);
                set += (unsigned)__popcll(v);
                store_word(a.dst + ((size_t)f * a.g.height + y) * (size_t)a.rb + (size_t)k * 8, v, a.vec_dst, a.rb, k);
            }
        } else {
            __syncthreads(); // the last trip has read its LDS
            for (int i = threadIdx.x; i < sh * kSW; i += kBlock) {
                const int sy = i / kSW, sx = i - sy * kSW;
                s_a[i] = morph_load(a.src, a.src_plane, a.vec_src, a.g, a.rb, (int)f, y0 - halo + sy, k0 - 1 + sx, 0ull);
            }
            __syncthreads();
            const uint64_t *from = s_a;
            uint64_t *to = s_b;
            unsigned core = 0, it = a.i0; // this lane's deletions among the tile's own pixels in iteration `it`
            int any = 0;                  // this lane deleted something in the staged region in this full iteration
            for (int s = 0; s < a.n_sub; s++) {
                const int sub = (a.sub0 + s) & 1;
                for (int i = threadIdx.x; i < sh * kSW; i += kBlock) {
                    const int sy = i / kSW, sx = i - sy * kSW;
                    const bool up = sy > 0, down = sy + 1 < sh, left = sx > 0, right = sx + 1 < kSW; // beyond: 0
                    const uint64_t *p = from + i;
                    const uint64_t mc = p[0];
                    if (mc == 0) { // nothing to delete; a wave whose words are all empty does no more than this
                        to[i] = 0;
                        continue;
                    }
                    const uint64_t ul = up && left ? p[-kSW - 1] : 0ull, uc = up ? p[-kSW] : 0ull, ur = up && right ? p[-kSW + 1] : 0ull;
                    const uint64_t ml = left ? p[-1] : 0ull, mr = right ? p[1] : 0ull;
                    const uint64_t dl = down && left ? p[kSW - 1] : 0ull, dc = down ? p[kSW] : 0ull,
                                   dr = down && right ? p[kSW + 1] : 0ull;
                    // every pixel of the word with its eight neighbours set: neither method deletes such a pixel (B = 8; C = 0)
                    if ((mc & uc & dc) == ~0ull && (((ul & ml & dl) >> 63) & ur & mr & dr & 1ull)) {
                        to[i] = mc;
                        continue;
                    }
                    const uint64_t del = thin_deletions<METHOD>(mc, uc, funnel(ul, uc, ur, 1), funnel(ml, mc, mr, 1),
                                                                funnel(dl, dc, dr, 1), dc, funnel(dl, dc, dr, -1),
                                                                funnel(ml, mc, mr, -1), funnel(ul, uc, ur, -1), sub);
                    to[i] = mc & ~del;
                    any |= del != 0;
                    if (sy >= halo && sy < halo + th && sx >= 1 && sx <= kTW) core += (unsigned)__popcll(del);
                }
                const bool iteration_ends = sub == 1 || s == a.n_sub - 1;
                if (iteration_ends) {
                    core = wave_sum(core);
                    if (lane0 && core) atomicAdd(a.del_cur + (size_t)f * kChunk + (it - a.chunk_i0), (unsigned long long)core);
                    core = 0, it++;
                }
                const uint64_t *const tmp = to;
                to = const_cast<uint64_t *>(from), from = tmp;
                if (sub == 1 && a.sub0 == 0) { // a full iteration of a fused launch ends (the same on every lane)
                    if (!__syncthreads_or(any)) break; // a fixed point of the staged region: the rest would change nothing
                    any = 0;
                } else {
                    __syncthreads();
                }
            }
            for (int i = threadIdx.x; i < th * kTW; i += kBlock) {
                const int oy = i / kTW, ox = i - oy * kTW;
                const int y = y0 + oy, k = k0 + ox;
                if (k >= a.g.tiles_x) continue;
                const uint64_t v = from[(halo + oy) * kSW + 1 + ox]; // pad bits and words outside were staged 0 and stay 0
                set += (unsigned)__popcll(v);
                store_word(a.dst + ((size_t)f * a.g.height + y) * (size_t)a.rb + (size_t)k * 8, v, a.vec_dst, a.rb, k);
            }
        }
        if (a.state) {
            set = wave_sum(set);
            if (lane0 && set) atomicAdd(a.state + (size_t)f * 4, (unsigned long long)set);
        }
    }
}

// Behind a chunk: the frame's iterations that deleted something and their deletions into its state; *active counts the frames
// whose n_used iterations all deleted something -- the ones that have not reported a fixed point yet.
__global__ __launch_bounds__(kBlock) void thin_fold_kernel(const unsigned long long *del, int n_frames, int n_used,
                                                           unsigned long long *state, unsigned long long *active)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_frames) return;
    unsigned long long nz = 0, sum = 0;
    for (int j = 0; j < n_used; j++) {
        const unsigned long long v = del[(size_t)f * kChunk + j];
        nz += v != 0, sum += v;
    }
    state[(size_t)f * 4 + 1] += nz; // one writer a frame
    state[(size_t)f * 4 + 2] += sum;
    if (active && nz == (unsigned long long)n_used) atomicAdd(active, 1ull);
}

__global__ __launch_bounds__(kBlock) void thin_info_kernel(const unsigned long long *state, int n_frames, int max_iterations,
                                                           long long *info)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_frames) return;
    const unsigned long long *s = state + (size_t)f * 4;
    long long *r = info + (size_t)f * 4;
    r[0] = (long long)s[0], r[1] = (long long)s[1], r[2] = (long long)s[2];
    r[3] = max_iterations == 0 || s[1] < (unsigned long long)max_iterations;
}

bool vec_map(const void *p, int rb) { return !(rb & 7) && !((uintptr_t)p & 7); }

size_t map_slot(int n_frames, int h, int w) { return ((size_t)n_frames * h * ((w + 7) / 8) + 15) & ~(size_t)15; }
size_t ring_half(int n_frames) { return (size_t)n_frames * kChunk; } // words

// The parts of the workspace
struct ThinWs {
    uint8_t *map[2];
    unsigned long long *ring, *state, *active;
    ThinWs(void *ws, int n_frames, int h, int w)
    {
        const size_t slot = map_slot(n_frames, h, w);
        map[0] = (uint8_t *)ws, map[1] = map[0] + slot;
        ring = (unsigned long long *)(map[1] + slot);
        state = ring + 2 * ring_half(n_frames);
        active = state + (size_t)n_frames * 4;
    }
};

} // namespace

LaunchPlan plan_thin_tiles(int n_frames, int h, int w)
{
    const unsigned long long words = ((unsigned long long)w + 63) / 64;
    const unsigned long long tiles = ((words + kTW - 1) / kTW) * (((unsigned long long)h + kTH - 1) / kTH);
    return capped_plan(tiles * (unsigned long long)n_frames, 1, kGridCap);
}

int thin_auto_fuse() { return kAutoFuse; }

size_t thin_workspace_bytes(int n_frames, int h, int w)
{
    return 2 * map_slot(n_frames, h, w) + (2 * ring_half(n_frames) + (size_t)n_frames * 4 + 1) * sizeof(unsigned long long);
}

hipError_t launch_thin_zero(void *ws, int n_frames, int h, int w, long long *info, hipStream_t stream)
{
    const ThinWs s(ws, n_frames, h, w);
    hipError_t e = hipMemsetAsync(s.state, 0, ((size_t)n_frames * 4 + 1) * sizeof(unsigned long long), stream); // and *active
    if (e == hipSuccess && info) e = hipMemsetAsync(info, 0, (size_t)n_frames * 4 * sizeof(long long), stream);
    return e;
}

hipError_t launch_thin_passes(const void *src, bool src_plane, int n_frames, int h, int w, int method, int max_iterations,
                              int route, int fuse, void *ws, uint8_t *out, hipStream_t stream)
{
    if (!src || !out || !ws || n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || method < 0 ||
        method > 1 || max_iterations < 0 || max_iterations > 16384 || route < 0 || route > 2 || fuse < 0 || fuse > kMaxFuse)
        return hipErrorInvalidValue;
    // full iterations a launch: 0 is the stepwise route
    int F = 0;
    if (route == 2) // asked for by name: automatic's fuse, or kFusedDefault should automatic ever be the stepwise route
        F = fuse ? fuse : (kAutoFuse ? kAutoFuse : kFusedDefault);
    else if (route == 0 && kAutoFuse)
        F = fuse ? fuse : kAutoFuse;
    const ThinWs s(ws, n_frames, h, w);
    const LaunchPlan p = plan_thin_tiles(n_frames, h, w);
    const HystGeom g = make_hyst_geom(h, w, n_frames);
    ThinArgs a;
    a.g = g, a.rb = (w + 7) / 8;
    a.n_units = p.units, a.trips = (unsigned)p.trips();
    a.tiles_x = (unsigned)((g.tiles_x + kTW - 1) / kTW), a.tiles_y = (unsigned)((h + kTH - 1) / kTH);
    const void *from = src;
    bool plane = src_plane;
    unsigned n_launch = 0;
    // one launch: n_sub sub-iterations from parity sub0 of iteration i0; last: into the caller's output, counting its bits
    auto launch = [&](unsigned i0, unsigned chunk_i0, int half, int prev_off, int sub0, int n_sub, bool last) {
        uint8_t *to = last ? out : s.map[n_launch++ & 1];
        a.src = from, a.dst = to, a.src_plane = plane, a.vec_src = !plane && vec_map(from, a.rb), a.vec_dst = vec_map(to, a.rb);
        a.del_cur = s.ring + (size_t)half * ring_half(n_frames), a.del_prev = s.ring + (size_t)(half ^ 1) * ring_half(n_frames);
        a.state = last ? s.state : nullptr;
        a.sub0 = sub0, a.n_sub = n_sub, a.i0 = i0, a.chunk_i0 = chunk_i0, a.prev_off = prev_off;
        if (method == 0)
            hipLaunchKernelGGL((thin_kernel<0>), dim3(p.grid), dim3(kBlock), 0, stream, a);
        else
            hipLaunchKernelGGL((thin_kernel<1>), dim3(p.grid), dim3(kBlock), 0, stream, a);
        from = to, plane = false;
        return hipGetLastError();
    };
    hipError_t e = hipSuccess;
    unsigned done = 0; // iterations queued
    int half = 0, prev_len = 0, want = 8;
    const dim3 fgrid((unsigned)((n_frames + kBlock - 1) / kBlock));
    for (;;) {
        const int len = max_iterations ? min(want, max_iterations - (int)done) : want;
        const bool last_chunk = max_iterations && done + (unsigned)len == (unsigned)max_iterations;
        unsigned long long *cur = s.ring + (size_t)half * ring_half(n_frames);
        if ((e = hipMemsetAsync(cur, 0, ring_half(n_frames) * sizeof(unsigned long long), stream)) != hipSuccess) return e;
        for (int j = 0; j < len && e == hipSuccess;) {
            if (F == 0) {
                e = launch(done + j, done, half, prev_len - 1, 0, 1, false);
                if (e == hipSuccess) e = launch(done + j, done, half, prev_len - 1, 1, 1, last_chunk && j + 1 == len);
                j++;
            } else {
                const int n = min(F, len - j);
                e = launch(done + j, done, half, prev_len - 1, 0, 2 * n, last_chunk && j + n == len);
                j += n;
            }
        }
        if (e != hipSuccess) return e;
        if (!max_iterations && (e = hipMemsetAsync(s.active, 0, sizeof(unsigned long long), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(thin_fold_kernel, fgrid, dim3(kBlock), 0, stream, cur, n_frames, len, s.state,
                           max_iterations ? nullptr : s.active);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        done += (unsigned)len, prev_len = len, half ^= 1, want = min(2 * want, kChunk);
        if (last_chunk) return hipSuccess;
        if (!max_iterations) {
            unsigned long long active = 0;
            if ((e = hipMemcpyAsync(&active, s.active, sizeof(active), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            if (!active) break;
        }
    }
    // every frame has reported its fixed point: every workgroup of this launch takes the copy path into the caller's output
    return launch(done, done, half, prev_len - 1, 0, 2, true);
}

hipError_t launch_thin_info(void *ws, int n_frames, int h, int w, int max_iterations, long long *info, hipStream_t stream)
{
    if (!info) return hipSuccess;
    const ThinWs s(ws, n_frames, h, w);
    hipLaunchKernelGGL(thin_info_kernel, dim3((unsigned)((n_frames + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, s.state,
                       n_frames, max_iterations, info);
    return hipGetLastError();
}

} // namespace canny
