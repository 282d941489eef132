// canny_reconstruct.hip -- morphological reconstruction by dilation of packed bit maps: a start set flooded inside a set G that
// conducts, to the fixed point (seeded reconstruction, fill holes, clear border).  The rule is part of the interface
// (include/canny_hip.h); tests/reconstruct_rule.py restates it in numpy, canny_reconstruct_host.cpp as a
// stack flood in plain C++.  All bit operations; the only atomics are integer sums and counts of waves that changed something,
// with no order to depend on.  The fixed point is unique: the same bytes on every run, route and machine.
//
//   state     : one 64-bit word per 64 columns, in the byte order of the packed layout (flip_bits <-> LSB-first).  Where the
//               rows of the caller's output are whole aligned words it lives IN the output; otherwise in a word-aligned copy
//               at the head of the workspace, and the finish kernel writes the output's bytes.
//   G         : the mask's word (SEEDED, CLEAR_BORDER) or its in-frame complement (FILL_HOLES), formed where the words are
//               formed: no lane tests a pixel.
//   init      : a lane per word: the start set into the state, its set bits and the mask's into the accumulators.
//   tile flood: a workgroup of 256 per tile of 8 words x 64 rows and trip of a capped grid: G of the tile and the state of the
//               tile plus one row above and below and one word left and right to LDS; rounds of "s |= n & g, then the flood
//               within the word" (canny_recon_words.h) until a round changes nothing; changed words back.
//   stepwise  : a lane per word, one geodesic dilation step through global memory: the cross-check.
//   finish    : a lane per word: the op's output from the state, pad bits 0, its set bits; then one thread a frame writes info.
//   In place, and why that is sound: the state only grows and never beyond the fixed point, so a workgroup that reads a
//   neighbour's stale word is only delayed.  Words another workgroup may write during the launch are read and written with
//   relaxed agent-scope atomics on aligned 64-bit words.  A launch in which no wave changed anything saw a state that did not
//   change during the launch: the fixed point.
//   changed   : per frame and launch the waves that changed a word.  A workgroup that arrives at a frame whose preceding launch
//               (final by stream order) changed nothing returns at once.  Launches are queued in chunks of 4, 8, 16, 32, then
//               64; the words of a chunk live in one half of a ring of two; behind a chunk one thread a frame counts the frames
//               whose last launch still changed something into ONE word, which the host reads.
#include "canny_bit_words.h" // flip_bits, morph_load, store_word
#include "canny_kernels.h"
#include "canny_recon_words.h" // recon_fill, recon_vertical, recon_step

namespace canny {

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 8, kTH = 64; // tile: words (of 64 columns) x rows
constexpr int kSW = kTW + 2, kSH = kTH + 2;
constexpr unsigned kGridCap = 4096;
constexpr int kChunk = 64;       // launches of a chunk at most: the words of a frame in one half of the ring
constexpr int kFirstChunk = 4;
// Which route automatic takes: the tile flood.  Measured on the MI355X at 128 x 4K (DESIGN.md section 38,
// profiles/reconstruct.jsonl): FILL_HOLES of Otsu-binarized frames 10.7 ms against 630 stepwise, SEEDED on blobs 4.2 against 24.9.
constexpr int kAutoRoute = 2;

enum { OP_SEEDED = 0, OP_FILL = 1, OP_CLEAR = 2 };

struct ReconArgs {
    const void *mask;
    const uint8_t *marker;
    uint64_t *state;                 // [n_frames][h][sw] words in the packed layout's byte order
    uint8_t *out;
    unsigned long long *acc;         // [n_frames][3]: set bits of the output, of M, of the start set
    unsigned long long *chg_cur;     // [n_frames][kChunk]: the waves that changed a word, per launch of this chunk
    const unsigned long long *chg_prev;
    HystGeom g;                      // tiles_x = the words of a row
    int rb, sw;                      // bytes of a packed row, words of a row of the state
    unsigned long long n_units;
    unsigned trips, tiles_x, tiles_y; // tiles of the flood, not of g
    int mask_plane, vec_mask, vec_marker, vec_out;
    int op, eight;
    int j, prev_off;                 // the launch within its chunk; where the preceding chunk's last launch sits (-1: none)
};

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int o = 32; o; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

__device__ __forceinline__ uint64_t in_frame(const HystGeom &g, int k)
{
    const int left = g.width - (k << 6);
    return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}

// the mask's word; outside the frame 0
__device__ __forceinline__ uint64_t mask_word(const ReconArgs &a, int f, int y, int k)
{
    return morph_load(a.mask, a.mask_plane, a.vec_mask, a.g, a.rb, f, y, k, 0ull);
}

// the word of the set that conducts; y, k inside the frame
__device__ __forceinline__ uint64_t g_word(const ReconArgs &a, int f, int y, int k)
{
    const uint64_t m = mask_word(a, f, y, k);
    return a.op == OP_FILL ? ~m & in_frame(a.g, k) : m;
}

// the border ring's pixels of word k of row y
__device__ __forceinline__ uint64_t border_word(const HystGeom &g, int y, int k)
{
    if (y == 0 || y == g.height - 1) return in_frame(g, k);
    uint64_t b = k == 0 ? 1ull : 0ull;
    if (k == ((g.width - 1) >> 6)) b |= 1ull << ((g.width - 1) & 63);
    return b;
}

__device__ __forceinline__ uint64_t *state_at(const ReconArgs &a, int f, int y, int k)
{
    return a.state + ((size_t)f * a.g.height + y) * (size_t)a.sw + k;
}

// a word of the state as an LSB-first word; outside the frame 0.  Another workgroup may be writing it.
__device__ __forceinline__ uint64_t state_load(const ReconArgs &a, int f, int y, int k)
{
    if (y < 0 || y >= a.g.height || k < 0 || k >= a.g.tiles_x) return 0ull;
    return flip_bits(__hip_atomic_load(state_at(a, f, y, k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ void state_store(const ReconArgs &a, int f, int y, int k, uint64_t v)
{
    __hip_atomic_store(state_at(a, f, y, k), flip_bits(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the frame's preceding launch, final by stream order, changed nothing: the frame is at its fixed point
__device__ __forceinline__ bool frame_done(const ReconArgs &a, unsigned f)
{
    if (a.j > 0) return a.chg_cur[(size_t)f * kChunk + (a.j - 1)] == 0;
    if (a.prev_off >= 0) return a.chg_prev[(size_t)f * kChunk + a.prev_off] == 0;
    return false;
}

// adds a lane's counts to word `slot` of its frame: one atomic a wave where the wave lies in one frame
__device__ __forceinline__ void acc_add(unsigned long long *acc, bool live, unsigned f, int slot, unsigned v)
{
    const unsigned f0 = (unsigned)__shfl((int)f, 0);
    if (__all(!live || f == f0)) {
        const unsigned s = wave_sum(live ? v : 0u);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(acc + (size_t)f0 * 3 + slot, (unsigned long long)s);
    } else if (live && v) {
        atomicAdd(acc + (size_t)f * 3 + slot, (unsigned long long)v);
    }
}

// word index -> frame, row, word of the row
__device__ __forceinline__ void word_of(const ReconArgs &a, unsigned long long i, unsigned &f, int &y, int &k)
{
    const unsigned long long per_frame = (unsigned long long)a.g.height * a.g.tiles_x;
    f = (unsigned)(i / per_frame);
    const unsigned r = (unsigned)(i % per_frame);
    y = (int)(r / (unsigned)a.g.tiles_x), k = (int)(r % (unsigned)a.g.tiles_x);
}

__global__ __launch_bounds__(kBlock) void recon_init_kernel(ReconArgs a)
{
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long i = ((unsigned long long)trip * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        const bool live = i < a.n_units;
        unsigned f = 0, n_m = 0, n_s = 0;
        if (live) {
            int y, k;
            word_of(a, i, f, y, k);
            const uint64_t m = mask_word(a, (int)f, y, k);
            uint64_t s;
            if (a.op == OP_SEEDED)
                s = morph_load(a.marker, false, a.vec_marker, a.g, a.rb, (int)f, y, k, 0ull) & m;
            else
                s = (a.op == OP_FILL ? ~m & in_frame(a.g, k) : m) & border_word(a.g, y, k);
            *state_at(a, (int)f, y, k) = flip_bits(s);
            n_m = (unsigned)__popcll(m), n_s = (unsigned)__popcll(s);
        }
        acc_add(a.acc, live, f, 1, n_m);
        acc_add(a.acc, live, f, 2, n_s);
    }
}

__global__ __launch_bounds__(kBlock) void recon_finish_kernel(ReconArgs a)
{
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long i = ((unsigned long long)trip * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        const bool live = i < a.n_units;
        unsigned f = 0, n = 0;
        if (live) {
            int y, k;
            word_of(a, i, f, y, k);
            const uint64_t s = flip_bits(*state_at(a, (int)f, y, k)); // pad bits are 0: the state is a subset of the frame
            uint64_t v = s;
            if (a.op == OP_FILL) v = in_frame(a.g, k) & ~s;
            if (a.op == OP_CLEAR) v = mask_word(a, (int)f, y, k) & ~s;
            store_word(a.out + ((size_t)f * a.g.height + y) * (size_t)a.rb + (size_t)k * 8, v, a.vec_out, a.rb, k);
            n = (unsigned)__popcll(v);
        }
        acc_add(a.acc, live, f, 0, n);
    }
}

__global__ __launch_bounds__(kBlock) void recon_info_kernel(const unsigned long long *acc, int n_frames, long long *info)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_frames) return;
    for (int j = 0; j < 3; j++) info[(size_t)f * 3 + j] = (long long)acc[(size_t)f * 3 + j];
}

// Route 1: one geodesic dilation step of every word, in place.
__global__ __launch_bounds__(kBlock) void recon_step_kernel(ReconArgs a)
{
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long i = ((unsigned long long)trip * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        bool changed = false;
        unsigned f = 0;
        if (i < a.n_units) {
            int y, k;
            word_of(a, i, f, y, k);
            if (!frame_done(a, f)) {
                const uint64_t gw = g_word(a, (int)f, y, k);
                const uint64_t s = state_load(a, (int)f, y, k);
                if (gw != 0 && s != gw) {
                    const uint64_t l = state_load(a, (int)f, y, k - 1), r = state_load(a, (int)f, y, k + 1);
                    const uint64_t u = state_load(a, (int)f, y - 1, k), d = state_load(a, (int)f, y + 1, k);
                    uint64_t ul = 0, ur = 0, dl = 0, dr = 0;
                    if (a.eight) {
                        ul = state_load(a, (int)f, y - 1, k - 1), ur = state_load(a, (int)f, y - 1, k + 1);
                        dl = state_load(a, (int)f, y + 1, k - 1), dr = state_load(a, (int)f, y + 1, k + 1);
                    }
                    const uint64_t t = recon_step(s, gw, l, r, recon_vertical(ul, u, ur, dl, d, dr, a.eight));
                    if (t != s) {
                        state_store(a, (int)f, y, k, t);
                        changed = true;
                    }
                }
            }
        }
        // the lanes of a wave that changed something may lie in two frames: one count for each
        const unsigned f0 = (unsigned)__shfl((int)f, 0);
        const bool first = changed && f == f0, other = changed && f != f0;
        if (__any(first) && (threadIdx.x & 63) == 0) atomicAdd(a.chg_cur + (size_t)f0 * kChunk + a.j, 1ull);
        if (other) atomicAdd(a.chg_cur + (size_t)f * kChunk + a.j, 1ull);
    }
}

// Route 2: every tile to its own fixed point behind a halo of the state as the launch found it.
__global__ __launch_bounds__(kBlock) void recon_flood_kernel(ReconArgs a)
{
    __shared__ uint64_t s_s[kSH * kSW]; // the state: row 0 and kSH - 1, word 0 and kSW - 1 are the halo
    __shared__ uint64_t s_g[kTH * kTW];
    const unsigned per_frame = a.tiles_x * a.tiles_y;
    for (unsigned trip = 0; trip < a.trips; trip++) {
        const unsigned long long u = (unsigned long long)blockIdx.x * a.trips + trip;
        if (u >= a.n_units) break; // the same on every lane
        const unsigned f = (unsigned)(u / per_frame), t = (unsigned)(u % per_frame);
        if (frame_done(a, f)) continue; // the same on every lane; the state is in place: nothing to copy
        const int k0 = (int)(t % a.tiles_x) * kTW, y0 = (int)(t / a.tiles_x) * kTH;
        __syncthreads(); // the last trip has read its LDS
        int any = 0, open = 0; // a staged word of the state is set; a word of the tile can still grow
        for (int i = threadIdx.x; i < kSH * kSW; i += kBlock) {
            const int sy = i / kSW, sx = i - sy * kSW;
            const int y = y0 - 1 + sy, k = k0 - 1 + sx;
            const uint64_t s = state_load(a, (int)f, y, k);
            s_s[i] = s;
            any |= s != 0;
            if (sy >= 1 && sy <= kTH && sx >= 1 && sx <= kTW) {
                const bool inside = y < a.g.height && k < a.g.tiles_x;
                const uint64_t gw = inside ? g_word(a, (int)f, y, k) : 0ull;
                s_g[(sy - 1) * kTW + (sx - 1)] = gw;
                open |= s != gw;
            }
        }
        const int any_all = __syncthreads_or(any); // also: the staging is complete
        if (!any_all || !__syncthreads_or(open)) continue; // nothing to flood from, or nothing left to flood
        // this lane's words: i0 and i0 + kBlock of the tile's 512
        uint64_t first[2], cur[2];
        for (int q = 0; q < 2; q++) {
            const int i = threadIdx.x + q * kBlock;
            first[q] = cur[q] = s_s[(i / kTW + 1) * kSW + (i % kTW) + 1];
        }
        for (;;) {
            int moved = 0;
            uint64_t next[2];
            for (int q = 0; q < 2; q++) {
                const int i = threadIdx.x + q * kBlock;
                const uint64_t gw = s_g[i], s = cur[q];
                next[q] = s;
                if (gw == 0 || s == gw) continue; // nothing conducts, or everything that conducts is set
                const uint64_t *p = s_s + (i / kTW + 1) * kSW + (i % kTW) + 1;
                uint64_t ul = 0, ur = 0, dl = 0, dr = 0;
                if (a.eight) ul = p[-kSW - 1], ur = p[-kSW + 1], dl = p[kSW - 1], dr = p[kSW + 1];
                const uint64_t n = recon_vertical(ul, p[-kSW], ur, dl, p[kSW], dr, a.eight);
                next[q] = recon_fill(s | (n & gw), gw, p[-1] >> 63, p[1] & 1);
                moved |= next[q] != s;
            }
            __syncthreads(); // every lane has read the round's input
            for (int q = 0; q < 2; q++) {
                if (next[q] == cur[q]) continue;
                const int i = threadIdx.x + q * kBlock;
                s_s[(i / kTW + 1) * kSW + (i % kTW) + 1] = cur[q] = next[q];
            }
            if (!__syncthreads_or(moved)) break;
        }
        bool changed = false;
        for (int q = 0; q < 2; q++) {
            if (cur[q] == first[q]) continue; // such a word lies inside the frame: outside, G is 0
            const int i = threadIdx.x + q * kBlock;
            state_store(a, (int)f, y0 + i / kTW, k0 + i % kTW, cur[q]);
            changed = true;
        }
        if (__any(changed) && (threadIdx.x & 63) == 0) atomicAdd(a.chg_cur + (size_t)f * kChunk + a.j, 1ull);
    }
}

// Behind a chunk: *active counts the frames whose last launch of the chunk still changed something.
__global__ __launch_bounds__(kBlock) void recon_poll_kernel(const unsigned long long *chg, int n_frames, int n_used,
                                                            unsigned long long *active)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_frames) return;
    if (chg[(size_t)f * kChunk + (n_used - 1)] != 0) atomicAdd(active, 1ull);
}

bool vec_map(const void *p, int rb) { return !(rb & 7) && !((uintptr_t)p & 7); }

int words_of_row(int w) { return (w + 63) / 64; }
size_t ring_half(int n_frames) { return (size_t)n_frames * kChunk; } // words

// The parts of the workspace: a word-aligned copy of the state (used where the output's rows are not whole aligned words) |
// the ring | the accumulators | the poll word
struct ReconWs {
    uint64_t *copy;
    unsigned long long *ring, *acc, *active;
    ReconWs(void *ws, int n_frames, int h, int w)
    {
        copy = (uint64_t *)ws;
        ring = (unsigned long long *)(copy + (size_t)n_frames * h * words_of_row(w));
        acc = ring + 2 * ring_half(n_frames);
        active = acc + (size_t)n_frames * 3;
    }
};

LaunchPlan plan_words(int n_frames, int h, int w)
{
    return capped_plan((unsigned long long)n_frames * h * words_of_row(w), kBlock, kGridCap);
}

} // namespace

LaunchPlan plan_reconstruct(int n_frames, int h, int w, int route)
{
    if ((route ? route : kAutoRoute) == 1) return plan_words(n_frames, h, w);
    const unsigned long long words = (unsigned long long)words_of_row(w);
    const unsigned long long tiles = ((words + kTW - 1) / kTW) * (((unsigned long long)h + kTH - 1) / kTH);
    return capped_plan(tiles * (unsigned long long)n_frames, 1, kGridCap);
}

int reconstruct_auto_route() { return kAutoRoute; }

size_t reconstruct_workspace_bytes(int n_frames, int h, int w)
{
    return ((size_t)n_frames * h * words_of_row(w) + 2 * ring_half(n_frames) + (size_t)n_frames * 3 + 1) * sizeof(uint64_t);
}

hipError_t launch_reconstruct(int phase, const uint8_t *marker, const void *mask, bool mask_plane, int n_frames, int h, int w,
                              int op, int connectivity, int route, void *ws, uint8_t *out, long long *info, int *launches,
                              hipStream_t stream)
{
    if (!mask || !out || !ws || n_frames < 1 || n_frames > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || op < 0 ||
        op > 2 || (connectivity != 4 && connectivity != 8) || route < 0 || route > 2 || (op == OP_SEEDED) != (marker != nullptr))
        return hipErrorInvalidValue;
    const int r = route ? route : kAutoRoute;
    const ReconWs s(ws, n_frames, h, w);
    const LaunchPlan pw = plan_words(n_frames, h, w), pt = plan_reconstruct(n_frames, h, w, 2);
    ReconArgs a;
    a.mask = mask, a.marker = marker, a.out = out, a.acc = s.acc;
    a.g = make_hyst_geom(h, w, n_frames), a.rb = (w + 7) / 8;
    a.mask_plane = mask_plane, a.vec_mask = !mask_plane && vec_map(mask, a.rb);
    a.vec_marker = marker && vec_map(marker, a.rb), a.vec_out = vec_map(out, a.rb);
    a.state = a.vec_out ? reinterpret_cast<uint64_t *>(out) : s.copy;
    a.sw = words_of_row(w); // = rb / 8 where the output's rows are whole words
    // FILL_HOLES floods the background, which takes the dual connectivity
    a.op = op, a.eight = (op == OP_FILL ? 12 - connectivity : connectivity) == 8;
    a.tiles_x = (unsigned)((a.g.tiles_x + kTW - 1) / kTW), a.tiles_y = (unsigned)((h + kTH - 1) / kTH);
    a.chg_cur = s.ring, a.chg_prev = s.ring, a.j = 0, a.prev_off = -1;
    auto words_launch = [&](void (*kernel)(ReconArgs)) {
        a.n_units = pw.units, a.trips = (unsigned)pw.trips();
        hipLaunchKernelGGL(kernel, dim3(pw.grid), dim3(kBlock), 0, stream, a);
        return hipGetLastError();
    };
    hipError_t e;
    const dim3 fgrid((unsigned)((n_frames + kBlock - 1) / kBlock));
    if (phase == RECON_INIT) { // every word of the workspace that is read is zeroed or written first, in stream order
        e = hipMemsetAsync(s.acc, 0, ((size_t)n_frames * 3 + 1) * sizeof(unsigned long long), stream); // and *active
        if (e == hipSuccess && info) e = hipMemsetAsync(info, 0, (size_t)n_frames * 3 * sizeof(long long), stream);
        return e == hipSuccess ? words_launch(recon_init_kernel) : e;
    }
    if (phase == RECON_FINISH) {
        if ((e = words_launch(recon_finish_kernel)) != hipSuccess) return e;
        if (info) {
            hipLaunchKernelGGL(recon_info_kernel, fgrid, dim3(kBlock), 0, stream, s.acc, n_frames, info);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        return hipStreamSynchronize(stream); // as documented: the stream is idle when the call returns
    }
    if (launches) *launches = 0;
    int half = 0, prev_len = 0, want = kFirstChunk, n_launch = 0;
    for (;;) {
        unsigned long long *cur = s.ring + (size_t)half * ring_half(n_frames);
        if ((e = hipMemsetAsync(cur, 0, ring_half(n_frames) * sizeof(unsigned long long), stream)) != hipSuccess) return e;
        a.chg_cur = cur, a.chg_prev = s.ring + (size_t)(half ^ 1) * ring_half(n_frames), a.prev_off = prev_len - 1;
        for (int j = 0; j < want; j++, n_launch++) {
            a.j = j;
            if (r == 1) {
                e = words_launch(recon_step_kernel);
            } else {
                a.n_units = pt.units, a.trips = (unsigned)pt.trips();
                hipLaunchKernelGGL(recon_flood_kernel, dim3(pt.grid), dim3(kBlock), 0, stream, a);
                e = hipGetLastError();
            }
            if (e != hipSuccess) return e;
        }
        if ((e = hipMemsetAsync(s.active, 0, sizeof(unsigned long long), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(recon_poll_kernel, fgrid, dim3(kBlock), 0, stream, cur, n_frames, want, s.active);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        unsigned long long active = 0;
        if ((e = hipMemcpyAsync(&active, s.active, sizeof(active), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        if (launches) *launches = n_launch;
        if (!active) break;
        prev_len = want, half ^= 1, want = min(2 * want, kChunk);
    }
    return hipSuccess;
}

} // namespace canny
