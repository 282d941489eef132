// canny_capi.hip -- implementation of the C ABI declared in include/canny_hip.h.
//
// Host-side runtime around the kernels in canny_kernels.hip: contexts (one device + one stream),
// device workspaces that grow on demand and are reused across calls, HIP-event stage timers, the
// hysteresis convergence loop, the stream-overlapped batch path and the per-GPU sharder.
// There is no CPU implementation behind any of these entry points: without a HIP device every
// call fails with CANNY_HIP_ERR_NO_DEVICE.
#include "canny_hip.h"
#include "canny_kernels.h"

#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cctype>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

using namespace canny;

// HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a
// queue serialise.  The batch pipeline needs its upload, compute and download streams on separate queues beside
// whatever streams the host application has (measured: 25.3 -> 16.7 Gpix/s with six streams on four queues).  The
// variable belongs to the APPLICATION: it has to be in the environment before the HIP runtime initialises
// (bench.py and Main set it).  The library does not touch the process environment (round 2 did, from
// a constructor: a process-wide side effect that raced getenv() in other threads of a plugin host).

namespace {

// "0-3,8,10-11" -> cpu_set_t; returns the number of CPUs set (0 on a malformed list)
int parse_cpulist(const char *text, cpu_set_t *set)
{
    CPU_ZERO(set);
    int count = 0;
    const char *p = text;
    while (*p) {
        while (*p == ' ' || *p == ',' || *p == '\n' || *p == '\t') p++;
        if (!*p) break;
        char *end = nullptr;
        long a = std::strtol(p, &end, 10);
        if (end == p || a < 0) return 0;
        long b = a;
        p = end;
        if (*p == '-') {
            p++;
            b = std::strtol(p, &end, 10);
            if (end == p || b < a) return 0;
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) {
            CPU_SET((int)c, set);
            count++;
        }
    }
    return count;
}

// CPUs local to a GPU, from sysfs (/sys/bus/pci/devices/<bdf>/local_cpulist, e.g. "0-31,128-159")
bool device_local_cpus(int device, cpu_set_t *set)
{
    char bdf[32] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    for (char *c = bdf; *c; c++) *c = (char)std::tolower((unsigned char)*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/local_cpulist";
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f) return false;
    char line[4096] = {0};
    const bool got = std::fgets(line, sizeof line, f) != nullptr;
    std::fclose(f);
    if (!got) return false;
    return parse_cpulist(line, set) > 0;
}

// hipHostMalloc with the pages next to `device` (see canny_hip_host_alloc)
hipError_t numa_host_malloc(int device, void **host_ptr, size_t bytes)
{
    cpu_set_t local, saved;
    const bool rebind = device >= 0 && device_local_cpus(device, &local) &&
                        sched_getaffinity(0, sizeof saved, &saved) == 0 && sched_setaffinity(0, sizeof local, &local) == 0;
    hipError_t e = hipHostMalloc(host_ptr, bytes ? bytes : 1);
    if (e == hipSuccess && bytes) { // first touch, one byte per page
        volatile unsigned char *p = (volatile unsigned char *)*host_ptr;
        for (size_t off = 0; off < bytes; off += 4096) p[off] = 0;
    }
    if (rebind) (void)sched_setaffinity(0, sizeof saved, &saved);
    return e;
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need)
    {
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            bytes = 0;
            if (e != hipSuccess) return e;
        }
        // grow with a little head-room so slowly growing batches do not reallocate every call
        size_t want = need + need / 8;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            e = hipMalloc(&p, need);
            want = need;
        }
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct PinBuf { // page-locked host staging
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need, int device = -1)
    {
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = numa_host_malloc(device, &p, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// ---- host-side expansion of bit maps (the "compact" transfer of the batch pipelines) -------------------------------
// The edge map only ever holds EDGE and NOEDGE (src/utils.h:5-6), so a batch call does not have to move the
// reference's 2 bytes per pixel over PCIe: the device packs the finished map into one bit per pixel (rows MSB-first,
// padded to bytes: launch_edges_to_bits), that travels -- 1/16 of the s16 map --, and a small pool of host threads
// writes the caller's short (or byte) plane from it: one 16-byte (8-byte) streaming store per bit-map byte out of a
// 256-entry table.  The s16 batch was bound by the DOWNLOAD (51 GB/s D2H for 25.5 Gpix/s); this way it runs at the
// rate frames can be UPLOADED, like the bit-map API, and the caller still gets the reference's plane, bit for bit.
class ExpandPool {
public:
    struct Job {
        const uint8_t *bits; // bit rows of the block (row_bytes each) -- or, for a copy job, the source bytes
        void *dst;           // first pixel of the block in the caller's plane -- or the copy's destination
        int rows, width, row_bytes;
        bool to_u8;          // bytes instead of shorts
        std::atomic<int> *left; // jobs of the chunk still to do
        size_t copy_bytes = 0;  // != 0: a plain memcpy of that many bytes (staging of pageable input frames)
    };
    // dst[0, bytes) = src[0, bytes), split over the pool in 1 MB pieces; returns when it is done (the caller works too)
    void parallel_copy(void *dst, const void *src, size_t bytes)
    {
        constexpr size_t kPiece = 1u << 20;
        const int n = (int)((bytes + kPiece - 1) / kPiece);
        if (n <= 1) {
            std::memcpy(dst, src, bytes);
            return;
        }
        std::atomic<int> left{n};
        for (int i = 0; i < n; i++) {
            Job j{};
            j.bits = (const uint8_t *)src + (size_t)i * kPiece;
            j.dst = (uint8_t *)dst + (size_t)i * kPiece;
            j.copy_bytes = std::min(kPiece, bytes - (size_t)i * kPiece);
            j.left = &left;
            submit(j);
        }
        wait(left);
    }
    explicit ExpandPool(int n_threads)
    {
        for (int b = 0; b < 256; b++)
            for (int k = 0; k < 8; k++) {
                const bool on = (b & (0x80 >> k)) != 0; // MSB first: bit 7 is the row's first pixel of this byte
                lut16_[b][k] = on ? 255 : 0;            // EDGE / NOEDGE
                lut8_[b][k] = on ? 255 : 0;
            }
        for (int i = 0; i < n_threads; i++) threads_.emplace_back([this] { loop(); });
    }
    ~ExpandPool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_job_.notify_all();
        for (auto &t : threads_) t.join();
    }
    int size() const { return (int)threads_.size(); }
    void submit(const Job &j)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(j);
        }
        cv_job_.notify_one();
    }
    // blocks until `left` has reached zero; the waiting thread works on queued jobs meanwhile
    void wait(std::atomic<int> &left)
    {
        while (left.load(std::memory_order_acquire) > 0) {
            Job j;
            bool have = false;
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (!q_.empty()) {
                    j = q_.front();
                    q_.pop_front();
                    have = true;
                }
            }
            if (have) {
                run(j);
            } else {
                std::unique_lock<std::mutex> lk(mu_);
                cv_done_.wait_for(lk, std::chrono::microseconds(50),
                                  [&] { return left.load(std::memory_order_acquire) <= 0 || !q_.empty(); });
            }
        }
    }

private:
    void loop()
    {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_job_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return; // stop_
                j = q_.front();
                q_.pop_front();
            }
            run(j);
        }
    }
    void run(const Job &j)
    {
        if (j.copy_bytes) std::memcpy(j.dst, j.bits, j.copy_bytes);
        for (int r = 0; r < (j.copy_bytes ? 0 : j.rows); r++) {
            const uint8_t *src = j.bits + (size_t)r * j.row_bytes;
            const int full = j.width / 8, tail = j.width % 8;
            if (j.to_u8) {
                uint8_t *d = (uint8_t *)j.dst + (size_t)r * j.width;
                for (int b = 0; b < full; b++) std::memcpy(d + 8 * b, lut8_[src[b]], 8);
                if (tail) std::memcpy(d + 8 * full, lut8_[src[full]], tail);
            } else {
                short *d = (short *)j.dst + (size_t)r * j.width;
#if defined(__SSE2__)
                if ((((uintptr_t)d) & 15) == 0) { // streaming stores: the plane is written once and not read here
                    for (int b = 0; b < full; b++)
                        _mm_stream_si128((__m128i *)(d + 8 * b), _mm_load_si128((const __m128i *)lut16_[src[b]]));
                } else
#endif
                {
                    for (int b = 0; b < full; b++) std::memcpy(d + 8 * b, lut16_[src[b]], 16);
                }
                if (tail) std::memcpy(d + 8 * full, lut16_[src[full]], 2 * tail);
            }
        }
#if defined(__SSE2__)
        _mm_sfence();
#endif
        if (j.left->fetch_sub(1, std::memory_order_acq_rel) == 1) {
            std::lock_guard<std::mutex> lk(mu_); // pairs with wait(): no lost wake-up
            cv_done_.notify_all();
        }
    }
    alignas(16) short lut16_[256][8];
    alignas(8) uint8_t lut8_[256][8];
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_job_, cv_done_;
    std::deque<Job> q_;
    bool stop_ = false;
};

struct EventPair {
    hipEvent_t a, b;
};

// One propagation in flight: a frame range with its planes, scheduling words, flags and the stream it runs on.
struct PropLane {
    hipStream_t stream = nullptr;
    uint64_t *S = nullptr;
    const uint64_t *C = nullptr;
    unsigned *sched = nullptr, *flags = nullptr; // device: tile stamps + queues + counters; last_change, domain
    unsigned *host = nullptr, *host_dev = nullptr; // 4 pinned words: last_change, domain, sequence number, spare
    hipEvent_t event = nullptr;                    // recorded behind every publish (fallback wait, stream join)
    HystGeom g{};
    short *edges = nullptr;
    int edge_value = 0;
    int iter = 0;       // sweeps launched so far
    unsigned seq = 0;   // sequence number of the last publish
    bool converged = false;
};

// The profile slots: the canny stages, then every feature's parts (canny_hip_<name>_profile_get), in this order.  A new
// feature adds a row at the end.
struct ProfGroup {
    const char *name;
    int parts;
};
constexpr ProfGroup kProfGroups[] = {
    {"stages", CANNY_HIP_STAGE_END},
    {"hough", 3},
    {"components", CANNY_HIP_CC_PARTS},
    {"edt", CANNY_HIP_EDT_PARTS},
    {"hough_segments", CANNY_HIP_SEGMENT_PARTS},
    {"contours", CANNY_HIP_CONTOUR_PARTS},
    {"hough_circles", CANNY_HIP_CIRCLE_PARTS},
    {"polygons", CANNY_HIP_POLYGON_PARTS},
    {"edgels", CANNY_HIP_EDGEL_PARTS},
    {"line_fits", CANNY_HIP_LINE_FIT_PARTS},
    {"circle_fits", CANNY_HIP_CIRCLE_FIT_PARTS},
    {"chamfer", CANNY_HIP_CHAMFER_PARTS},
    {"shapes", CANNY_HIP_SHAPE_PARTS},
    {"curves", CANNY_HIP_CURVE_PARTS},
    {"corners", CANNY_HIP_CORNER_PARTS},
    {"descriptors", CANNY_HIP_DESC_PARTS},
    {"motion", CANNY_HIP_MOTION_PARTS},
    {"warp", CANNY_HIP_WARP_PARTS},
    {"fuse", CANNY_HIP_FUSE_PARTS},
    {"morph", CANNY_HIP_MORPH_PARTS},
    {"binarize", CANNY_HIP_BIN_PARTS},
    {"thin", CANNY_HIP_THIN_PARTS},
    {"reconstruct", CANNY_HIP_RECON_PARTS},
    {"gray_morph", CANNY_HIP_GRAY_PARTS},
    {"pyramid", CANNY_HIP_PYR_PARTS},
};

// The first slot of the named group; with no name, the number of slots.  A name the table does not hold fails to compile.
constexpr int prof_base(const char *name)
{
    int base = 0;
    for (const ProfGroup &g : kProfGroups) {
        const char *a = g.name, *b = name;
        while (b && *a && *a == *b) a++, b++;
        if (b && *a == *b) return base;
        base += g.parts;
    }
    return name ? throw "no such profile group" : base;
}

// Every device workspace of a context but the staging blocks io[4]: canny_hip_ctx derives from this, so a workspace is
// ctx->name.  Nothing but DevBuf members may stand here, and each has its row in kWorkspaces below (DESIGN.md section 20
// has one too): the static_assert behind the table fails the build otherwise.
struct Workspaces {
    // device workspaces
    DevBuf tmp_f32;   // generic Gaussian row-pass plane
    DevBuf smoothed;  // pipeline: Gaussian output
    DevBuf edges16;   // canny_hip_dev_canny_u8: the s16 edge map before narrowing
    DevBuf gray;      // colour input: the converted plane when the Gaussian cannot convert itself
    DevBuf hist;      // automatic thresholds: per-frame histograms (n_frames x 257 u32)
    DevBuf thr;       // automatic thresholds: the pairs when the caller does not ask for them
    DevBuf points;    // edge point lists: per-frame totals (n_frames u64), then per-row counts / prefixes (u32)
    // Hough lines: the accumulators when the caller passes none; candidate keys, histograms, tie counts, cut words; the
    // vote tables on the device with the host copy they were sent from and the arguments they belong to
    DevBuf hough_accum, hough_ws, hough_tab;
    // connected components: the parent array (4 B/px) when the caller passes no label plane; per-frame totals and per-row
    // counts / prefixes of the numbering scan
    DevBuf cc_parent, cc_ws;
    // contour chains: per-frame totals and per-row sums / prefixes of the chain points (the scan's second use)
    DevBuf ct_ws;
    // polygon approximation: the vertex masks (8 B per record slot), the scan's block sums, the vertex flags of long chains
    // (1 B per point slot); the chains themselves when canny_hip_canny_polygons keeps them on the device
    DevBuf pg_ws, pg_points;
    // contour shape measures: per point slot the column extremes, the two lists of the hull's rounds and the finished hull
    // (20 B per point slot), then the scan's block sums
    DevBuf sh_ws;
    // distance transform: the row pass's u16 plane (2 B/px, rows padded to 64 pixels); the column scan's stack (4 B/px) when
    // the caller passes no dist2 plane to keep it in
    DevBuf edt_cols, edt_stack;
    // Hough segments: per-line counts and offsets; bases and line counts when the caller passes none; the private copy of
    // the map that exclusive mode clears pixels from
    DevBuf seg_ws, seg_lines, seg_work;
    // Hough circles: the accumulators when the caller passes none; candidate keys, votes, bases, radii, supports, peak
    // counts, histograms, tie counts, cut words
    DevBuf circ_accum, circ_ws;
    // circle fits: the circle records and counts when the caller passes none
    DevBuf circ_recs;
    // chamfer matching, per chunk of frames: the u16 cost plane; the scores when the caller passes no plane for them; the
    // candidate passes' keys, histograms and counters; and the dist2 plane of the whole batch when the caller passes none
    DevBuf chamfer_cost, chamfer_scores, chamfer_ws, chamfer_dist2;
    // corners, per chunk of frames: the collected keys, the radix select's state, the maxima, histograms and counters
    DevBuf corners_ws;
    // descriptor matching: the pairs as the kernels read them, then per (pair, train slot) its best query
    DevBuf desc_ws;
    // motion estimate: the compacted correspondences and their slots, the inlier counts per (pair, hypothesis), m, the pairs
    DevBuf motion_ws;
    // binary morphology: the two intermediate bit maps of a call of more than one primitive step, back to back; grey-level
    // morphology: its two intermediate u8 planes, the same way (every call sizes and writes what it reads)
    DevBuf morph_ws;
    // binarization: the histograms of the frames (OTSU) | the threshold of every frame
    DevBuf binarize_ws;
    // thinning: two maps | the deletions per frame and iteration | the frames' states (thin_workspace_bytes); reconstruction:
    // a word-aligned copy of the state | the changed words per frame and launch | the accumulators (reconstruct_workspace_bytes)
    DevBuf thin_ws;
    DevBuf plane_s, plane_c, stamps, flags; // hysteresis bit-planes / scheduling words
};

// The workspaces by name, in the order canny_hip_selftest_workspace reports them: what it lists and what
// canny_hip_ctx_destroy releases.  kind: CANNY_HIP_WS_*.
struct WsRow {
    const char *name;
    DevBuf Workspaces::*buf;
    int kind;
};
constexpr WsRow kWorkspaces[] = {
    {"tmp_f32", &Workspaces::tmp_f32, CANNY_HIP_WS_DATA},
    {"smoothed", &Workspaces::smoothed, CANNY_HIP_WS_DATA},
    {"edges16", &Workspaces::edges16, CANNY_HIP_WS_DATA},
    {"gray", &Workspaces::gray, CANNY_HIP_WS_DATA},
    {"hist", &Workspaces::hist, CANNY_HIP_WS_DATA},
    {"thr", &Workspaces::thr, CANNY_HIP_WS_DATA},
    {"points", &Workspaces::points, CANNY_HIP_WS_INDEX},           // row prefixes: the scatter's write offsets
    {"hough_accum", &Workspaces::hough_accum, CANNY_HIP_WS_DATA},
    {"hough_ws", &Workspaces::hough_ws, CANNY_HIP_WS_INDEX},       // cut words: the select pass's slot counters
    {"hough_tab", &Workspaces::hough_tab, CANNY_HIP_WS_CACHE},
    {"cc_parent", &Workspaces::cc_parent, CANNY_HIP_WS_INDEX},
    {"cc_ws", &Workspaces::cc_ws, CANNY_HIP_WS_INDEX},
    {"ct_ws", &Workspaces::ct_ws, CANNY_HIP_WS_INDEX},
    {"pg_ws", &Workspaces::pg_ws, CANNY_HIP_WS_INDEX},             // block sums of the vertex scan
    {"pg_points", &Workspaces::pg_points, CANNY_HIP_WS_INDEX},     // pixel indices the stage decodes
    // lists of columns that index the extremes; block sums of the hull scan
    {"sh_ws", &Workspaces::sh_ws, CANNY_HIP_WS_INDEX},
    {"edt_cols", &Workspaces::edt_cols, CANNY_HIP_WS_INDEX},       // reused as the column scan's stack of row numbers
    {"edt_stack", &Workspaces::edt_stack, CANNY_HIP_WS_INDEX},
    {"seg_ws", &Workspaces::seg_ws, CANNY_HIP_WS_INDEX},
    {"seg_lines", &Workspaces::seg_lines, CANNY_HIP_WS_INDEX},     // bases decode into table rows, counts bound loops
    {"seg_work", &Workspaces::seg_work, CANNY_HIP_WS_DATA},
    {"circ_accum", &Workspaces::circ_accum, CANNY_HIP_WS_DATA},
    {"circ_ws", &Workspaces::circ_ws, CANNY_HIP_WS_INDEX},         // bases address accumulator cells, peak counts bound loops
    {"circ_recs", &Workspaces::circ_recs, CANNY_HIP_WS_INDEX},     // radii and centres bound the fit's row walk, counts its grid
    {"chamfer_cost", &Workspaces::chamfer_cost, CANNY_HIP_WS_DATA},
    {"chamfer_scores", &Workspaces::chamfer_scores, CANNY_HIP_WS_DATA},
    // keys address score cells, totals bound the sort, counters hand out slots
    {"chamfer_ws", &Workspaces::chamfer_ws, CANNY_HIP_WS_INDEX},
    {"chamfer_dist2", &Workspaces::chamfer_dist2, CANNY_HIP_WS_INDEX}, // doubles as the column scan's stack (see edt_stack)
    // keys address pixels, totals bound the sort, counters hand out slots
    {"corners_ws", &Workspaces::corners_ws, CANNY_HIP_WS_INDEX},
    // the pairs address frames, the best queries are compared with indices
    {"desc_ws", &Workspaces::desc_ws, CANNY_HIP_WS_INDEX},
    // the pairs address frames, m bounds the lists, the slots address the flags
    {"motion_ws", &Workspaces::motion_ws, CANNY_HIP_WS_INDEX},
    {"morph_ws", &Workspaces::morph_ws, CANNY_HIP_WS_DATA},
    {"binarize_ws", &Workspaces::binarize_ws, CANNY_HIP_WS_DATA},
    {"thin_ws", &Workspaces::thin_ws, CANNY_HIP_WS_DATA},
    {"plane_s", &Workspaces::plane_s, CANNY_HIP_WS_DATA},
    {"plane_c", &Workspaces::plane_c, CANNY_HIP_WS_DATA},
    {"stamps", &Workspaces::stamps, CANNY_HIP_WS_INDEX},           // tile queues and their counters
    {"flags", &Workspaces::flags, CANNY_HIP_WS_DATA},
};
static_assert(sizeof(Workspaces) == sizeof(kWorkspaces) / sizeof(kWorkspaces[0]) * sizeof(DevBuf),
              "every DevBuf member of Workspaces needs its row in kWorkspaces (and nothing else may be a member)");

} // namespace

struct canny_hip_ctx : Workspaces {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;
    int last_hyst_iters = 0;
    int gaussian_path = 0;   // 0 auto, 1 generic, 2 march
    int sobel_nms_path = 0;  // 0 auto, 1 LDS tile, 2 march
    int tune_sobel_seg = 0;  // A/B knob of the marching Sobel+NMS kernel: rows per segment, 0 = automatic
    int fuse_classify = 1;   // canny(): Sobel+NMS emits the hysteresis bit-planes directly when it can
    // canny(): the smoothed plane between the Gaussian and the fused Sobel+NMS kernel as bytes (its values lie in
    // [0,255], src/utils.cpp:62): 0 = s16 plane, 1 = u8 plane
    int smoothed_u8 = 1; // canny(): the plane between the Gaussian and the fused Sobel+NMS as bytes (round 3 default)
    int last_canny_u8 = 0; // whether the last canny call really used it (window, taps and shape permitting)
    // (n_frames, height, width) of the batch whose smoothed plane that call left in `smoothed` (0: no call yet):
    // canny_hip_dev_edgels_at with d_plane == NULL reads it
    int last_canny_n = 0, last_canny_h = 0, last_canny_w = 0;
    // colour input (canny_hip_*_color): the conversion rule (0 OpenCV, 1 PIL), whether the Gaussian may convert as it
    // loads (1) or a standalone pass always converts first (0), and whether the last colour canny call fused
    int gray_rule = 0;
    int fuse_gray = 1;
    int last_fused_gray = 0;
    // canny(): after the two batch-wide sweeps, one launch with a workgroup per frame finishes the propagation
    // (launch_hyst_tail): no further launches, no host round trip, the call returns without waiting.
    // 1 (default) = for frames of up to kTailMaxTiles tiles, 0 = never (the multi-launch scheme with its poll)
    int hyst_tail = 1;
    int hyst_tail_after = 2; // batch-wide sweeps before the tail kernel takes over (A/B: 2 or 3)
    bool hyst_iters_async = false; // last_hyst_iters has to be fetched from flags[0] (the tail path does not poll)
    // canny_hip_canny_batch: number of pipelines (host threads, each with an H2D, a compute and a D2H stream and a
    // ring of chunk slots) that each take every n-th chunk, and the chunk size (megabytes of input, or frames).
    // 0 = automatic, see canny_batch_impl.
    int batch_workers = 0;
    int batch_chunk_mb = 0;
    int batch_chunk_frames = 0;
    int batch_pipe_mode = 0; // 0 = automatic, 1 = three streams per pipeline, 2 = one in-order stream per pipeline
    // s16 / u8 batch maps travel as bit maps and are expanded by host threads (ExpandPool): 0 = automatic (on),
    // 1 = off (the map itself is downloaded, as in rounds 1-2); expand_threads: 0 = automatic
    int batch_compact = 0;
    int batch_expand_threads = 0;
    std::unique_ptr<ExpandPool> expand_pool;
    // the pipelines live as long as the context: creating a sub-context with its streams and allocating its
    // staging costs ~10 ms per call, a sixth of a 1024 x 1080p batch
    struct BatchPipe;
    std::vector<BatchPipe *> batch_pool;

    // the features' options and host-side state (their device workspaces are in Workspaces); an int option gets its row in
    // kOptions below.  Hough lines: the host copy the vote tables (hough_tab) were sent from, and the arguments they belong to
    std::vector<float> hough_tab_host;
    float hough_tab_key[3] = {0, 0, 0};
    int hough_tab_n = 0;
    int hough_path = 0;   // 0 auto (LDS rows when a row fits), 1 global atomics, 2 LDS rows
    int hough_lds_kb = 0; // A/B: LDS budget of a vote workgroup in KiB, 0 = automatic
    int chamfer_route = 0; // 0 auto, 1 direct, 2 tiled
    int warp_route = 0;    // 0 auto, 1 direct, 2 tiled
    int fuse_route = 0;    // the median of the temporal fusion: 0 auto, 1 registers, 2 passes
    int chamfer_chunk_mb = 0; // A/B and tests: budget of the score workspace in MiB, 0 = 256
    std::vector<canny_hip_chamfer_set *> chamfer_sets; // the sets created on this context and not yet destroyed
    std::vector<int> desc_pairs; // the validated pairs of the last match call: what its upload reads
    int morph_route = 0;   // 0 auto, 1 general, 2 separable (full rectangles)
    int binarize_route = 0; // 0 auto, 1 straightforward, 2 marching (ADAPTIVE_MEAN)
    int thin_route = 0, thin_fuse = 0; // 0 auto, 1 stepwise, 2 fused; 0 auto, 1..8 full iterations a fused launch
    int reconstruct_route = 0;         // 0 auto, 1 stepwise, 2 tile flood
    int last_reconstruct_launches = 0; // the sweep launches the last reconstruction call queued: a diagnostic
    int gray_morph_route = 0;          // 0 auto, 1 general, 2 fast (full rectangles separably, the median by a network)
    int pyramid_route = 0;             // 0 auto, 1 direct, 2 tiled
    std::vector<int> motion_pairs; // the validated pairs of the last motion call: what its upload reads
    DevBuf io[4];     // staging for the host-pointer stage functions
    std::string ws_name; // canny_hip_selftest_workspace: the name it handed out last
    unsigned *host_flags = nullptr;     // pinned + mapped, 4 words per lane: last_change, domain, sequence number, spare
    unsigned *host_flags_dev = nullptr; // the same memory as the device sees it
    unsigned publish_seq = 0;           // sequence number of the last launch_hyst_publish
    hipEvent_t flag_event = nullptr;    // recorded behind the publish kernel (fallback wait)
    // canny(), optional: the propagation of the first half of a batch runs on a second stream, beside the
    // Sobel+NMS kernel of the second half (the sweeps are latency bound and leave most of the chip idle).  Off by
    // default: 128 x 4K measured 2.76 ms with it against 2.72 ms without -- the Sobel+NMS kernel loses more
    // (two half-size launches, sweeps competing for its CUs) than the hidden sweeps give back.
    int overlap_hysteresis = 0;
    int stream_overlap = 0; // canny_hip_dev_canny_stream: sweeps on the second stream (see dev_canny_stream)
    hipStream_t aux_stream = nullptr;
    hipEvent_t fork_event = nullptr, aux_event = nullptr;
    // canny_hip_dev_canny_stream: the propagation of the batch submitted last, still in flight on aux_stream
    PropLane pend;
    bool has_pend = false;

    // profiling
    bool prof = false;
    unsigned prof_mask = ~0u; // stages whose launches get an event pair (each pair costs a few us of stream time)
    unsigned prof_every = 1;  // ... and only every prof_every-th launch group of a stage gets one
    // slots: kProfGroups in order; the aliases keep the call sites short
    static constexpr int kProfHough = prof_base("hough"), kProfComponents = prof_base("components"),
                         kProfEdt = prof_base("edt"), kProfSegments = prof_base("hough_segments"),
                         kProfContours = prof_base("contours"), kProfCircles = prof_base("hough_circles"),
                         kProfPolygons = prof_base("polygons"), kProfEdgels = prof_base("edgels"),
                         kProfLineFits = prof_base("line_fits"), kProfCircleFits = prof_base("circle_fits"),
                         kProfChamfer = prof_base("chamfer"), kProfShapes = prof_base("shapes"),
                         kProfCurves = prof_base("curves"), kProfCorners = prof_base("corners"),
                         kProfDescriptors = prof_base("descriptors"), kProfMotion = prof_base("motion"),
                         kProfWarp = prof_base("warp"), kProfFuse = prof_base("fuse"), kProfMorph = prof_base("morph"),
                         kProfBinarize = prof_base("binarize"), kProfThin = prof_base("thin"),
                         kProfReconstruct = prof_base("reconstruct"), kProfGrayMorph = prof_base("gray_morph"),
                         kProfPyramid = prof_base("pyramid");
    static constexpr int kProfSlots = prof_base(nullptr);
    // "profile_stage_mask" is a non-negative int option: bit 30 is the last it can carry
    static constexpr int kProfLastBit = 30;
    static_assert(prof_base("polygons") == kProfLastBit && prof_base("edgels") > kProfLastBit,
                  "profile_stage_mask has one bit per slot up to the polygon parts; every slot from there on follows bit 30");
    unsigned prof_seen[kProfSlots] = {0};
    std::vector<EventPair> pending[kProfSlots];
    std::vector<EventPair> pool;
    double total_ms[kProfSlots] = {0};
    long launches[kProfSlots] = {0};
};

namespace {

// The options that are a plain bounded load or store of an int member: canny_hip_ctx_get_option answers the readable
// ones, canny_hip_ctx_set_option stores a value in [min, max] into the writable ones.  Everything else (stream_overlap,
// the profile_* pair, the expand threads, the process-wide tune_* names) is explicit code behind the lookup.
struct OptRow {
    const char *name;
    int canny_hip_ctx::*field;
    int min, max;
    bool readable, writable;
};
constexpr OptRow kOptions[] = {
    {"gaussian_path", &canny_hip_ctx::gaussian_path, 0, 2, true, true},
    {"sobel_nms_path", &canny_hip_ctx::sobel_nms_path, 0, 2, true, true},
    {"tune_sobel_seg", &canny_hip_ctx::tune_sobel_seg, 0, 4096, false, true},
    {"fuse_classify", &canny_hip_ctx::fuse_classify, 0, 1, true, true},
    {"smoothed_u8", &canny_hip_ctx::smoothed_u8, 0, 1, true, true},
    {"last_canny_smoothed_u8", &canny_hip_ctx::last_canny_u8, 0, 0, true, false},
    {"gray_rule", &canny_hip_ctx::gray_rule, 0, 1, true, true},
    {"fuse_gray", &canny_hip_ctx::fuse_gray, 0, 1, true, true},
    {"last_canny_fused_gray", &canny_hip_ctx::last_fused_gray, 0, 0, true, false},
    {"hysteresis_tail", &canny_hip_ctx::hyst_tail, 0, 1, true, true},
    {"tune_hyst_tail_after", &canny_hip_ctx::hyst_tail_after, 1, 4, false, true},
    {"overlap_hysteresis", &canny_hip_ctx::overlap_hysteresis, 0, 1, false, true},
    {"tune_batch_workers", &canny_hip_ctx::batch_workers, 0, 16, false, true},
    {"tune_batch_chunk_mb", &canny_hip_ctx::batch_chunk_mb, 0, 1024, false, true},
    {"tune_batch_chunk_frames", &canny_hip_ctx::batch_chunk_frames, 0, 65535, false, true},
    {"tune_batch_pipe_mode", &canny_hip_ctx::batch_pipe_mode, 0, 2, false, true},
    {"tune_batch_compact", &canny_hip_ctx::batch_compact, 0, 1, true, true},
    {"hough_path", &canny_hip_ctx::hough_path, 0, 2, true, true},
    {"tune_hough_lds_kb", &canny_hip_ctx::hough_lds_kb, 0, kHoughLdsMax / 1024, true, true},
    {"chamfer_route", &canny_hip_ctx::chamfer_route, 0, 2, true, true},
    {"tune_chamfer_chunk_mb", &canny_hip_ctx::chamfer_chunk_mb, 0, 4096, true, true},
    {"warp_route", &canny_hip_ctx::warp_route, 0, 2, true, true},
    {"fuse_route", &canny_hip_ctx::fuse_route, 0, 2, true, true},
    {"morph_route", &canny_hip_ctx::morph_route, 0, 2, true, true},
    {"binarize_route", &canny_hip_ctx::binarize_route, 0, 2, true, true},
    {"thin_route", &canny_hip_ctx::thin_route, 0, 2, true, true},
    {"thin_fuse", &canny_hip_ctx::thin_fuse, 0, 8, true, true},
    {"reconstruct_route", &canny_hip_ctx::reconstruct_route, 0, 2, true, true},
    {"last_reconstruct_launches", &canny_hip_ctx::last_reconstruct_launches, 0, 0, true, false},
    {"gray_morph_route", &canny_hip_ctx::gray_morph_route, 0, 2, true, true},
    {"pyramid_route", &canny_hip_ctx::pyramid_route, 0, 2, true, true},
};

} // namespace

// One batch pipeline: three streams and a ring of chunk slots.  Chunk j of the pipeline lives in slot j % kSlots:
//   s_h2d:    host -> d_in                       (ev_h2d)
//   compute:  d_in -> d_out [-> d_out8]           (ev_comp; the sub-context's stream, waits for ev_h2d)
//   s_d2h:    d_out / d_out8 -> host              (ev_d2h; waits for ev_comp)
// so that the upload of chunk j+1, the kernels of chunk j and the download of chunk j-1 are in flight together and
// neither DMA engine waits for a host thread.  Pageable caller buffers go through the slot's pinned staging.
// HIP multiplexes a process's streams onto a handful of hardware queues (4 by default, GPU_MAX_HW_QUEUES), and
// streams that share a queue serialise: measured on 128 x 4K, the same pipeline ran at 25.3 Gpix/s with four streams
// alive in the process and at 16.7 with six.  So streams are created sparingly: pipeline 0 computes on the parent
// context itself (its stream is idle during a batch call), the copy streams exist only in three-stream mode.
struct canny_hip_ctx::BatchPipe {
    static constexpr int kSlots = 3;
    canny_hip_ctx *sub = nullptr; // compute context: the parent itself for pipeline 0, an owned sub-context otherwise
    bool owns_sub = false;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr; // three-stream mode only, created on first use
    struct Slot {
        DevBuf d_in, d_out, d_out8;
        PinBuf pin_in, pin_out;
        DevBuf d_thr;   // per-frame thresholds of the chunk (canny_hip_canny_batch_thresholds / _auto)
        PinBuf pin_thr; // ... staged: the chunk's explicit pairs on the way up, the selected pairs on the way down
        hipEvent_t ev_h2d = nullptr, ev_comp = nullptr, ev_d2h = nullptr;
        bool d2h_issued = false;      // ev_d2h has been recorded during the current call
        void *retire_dst = nullptr;   // pageable output: where pin_out goes once ev_d2h has fired
        size_t retire_bytes = 0;
        int retire_frames = 0;        // compact transfer: frames whose bit maps sit in pin_out
        std::atomic<int> expand_left{0}; // compact transfer: expansion jobs of this slot's chunk still running
    } slot[kSlots];
};

namespace {

int fail(canny_hip_ctx *ctx, hipError_t e, const char *where)
{
    if (ctx) {
        ctx->last_error = std::string(where) + ": " + hipGetErrorString(e);
    }
    (void)hipGetLastError();
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? CANNY_HIP_ERR_NO_DEVICE : CANNY_HIP_ERR_RUNTIME;
}

#define HIP_TRY(ctx, expr)                                  \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return fail((ctx), e_, #expr); \
    } while (0)

int bind(canny_hip_ctx *ctx)
{
    if (!ctx) return CANNY_HIP_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return CANNY_HIP_OK;
}

// RAII stage timer: brackets the launches of one stage with events on the launch stream.
struct StageTimer {
    canny_hip_ctx *ctx;
    int stage;
    EventPair ev{};
    bool on = false;
    hipStream_t stream;
    bool attach; // the events are not recorded around the launches but attached to ONE dispatch (launch_events())
    StageTimer(canny_hip_ctx *c, int s, hipStream_t on_stream = nullptr, bool attached = false)
        : ctx(c), stage(s), stream(on_stream ? on_stream : c->stream), attach(attached)
    {
        if (!ctx->prof || !(ctx->prof_mask >> (s < canny_hip_ctx::kProfLastBit ? s : canny_hip_ctx::kProfLastBit) & 1u)) return;
        if (ctx->prof_seen[s]++ % ctx->prof_every != 0) return;
        if (!ctx->pool.empty()) {
            ev = ctx->pool.back();
            ctx->pool.pop_back();
        } else {
            if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return;
        }
        on = attach || hipEventRecord(ev.a, stream) == hipSuccess;
    }
    LaunchEvents launch_events() const { return (on && attach) ? LaunchEvents{ev.a, ev.b} : LaunchEvents{}; }
    ~StageTimer()
    {
        if (!on) return;
        if (!attach) (void)hipEventRecord(ev.b, stream);
        ctx->pending[stage].push_back(ev);
    }
};

// createGaussianKernel, reference src/utils.cpp:77-95, evaluated on the host with the reference's
// exact expression types: float window rule, expf in float, the 1/(sqrt(2pi) sigma) factor in
// double, a float running sum and a float divide per tap.  (Built with -ffp-contract=off.)
int make_taps(float sigma, GaussTaps &t)
{
    if (!(sigma > 0.0f) || !std::isfinite(sigma)) return CANNY_HIP_ERR_INVALID;
    float wf = 1 + 2 * std::ceil(3 * sigma);
    if (!(wf >= 1.0f) || wf > (float)kMaxWindow) return CANNY_HIP_ERR_UNSUPPORTED;
    int window = (int)wf;
    int center = window / 2;
    float total = 0.0f;
    for (int i = 0; i < window; i++) {
        float x = (float)(i - center);
        float e = expf(-((x * x) / (2 * sigma * sigma)));
        float tap = (float)((double)e / (std::sqrt(6.2831853) * (double)sigma));
        t.tap[i] = tap;
        total += tap;
    }
    for (int i = 0; i < window; i++) t.tap[i] /= total;
    for (int i = window; i < kMaxWindow; i++) t.tap[i] = 0.0f;
    t.center = center;
    return CANNY_HIP_OK;
}

// What every canny_hip_selftest_*_plan export hands out of a launch plan: units, per_group, grid, trips, aux.
void store_plan(unsigned long long *out, const LaunchPlan &p)
{
    out[0] = p.units, out[1] = p.per_group, out[2] = p.grid, out[3] = p.trips(), out[4] = (unsigned long long)p.aux;
}

int check_dims(int height, int width, int n_frames)
{
    if (height < 1 || width < 1 || n_frames < 1) return CANNY_HIP_ERR_INVALID;
    if ((long long)height * width > 0x7fffffffLL) return CANNY_HIP_ERR_UNSUPPORTED;
    if (n_frames > 65535) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// Reached pixels are overwritten with EDGE = 255 while the reference's scan is still running (src/utils.cpp:327-334,
// 367).  With min_val > 255 such a pixel then fails the scan's own `< minVal` test when the scan reaches it and
// is zeroed again -- unless the scan has already passed it: the result depends on the scan order, which the
// parallel formulation does not have.  (If max_val > 255 as well everything ends as 0 either way.)
bool hysteresis_order_dependent(int min_val, int max_val) { return min_val > 255 && max_val <= 255; }

// Whether the last canny call ran on a batch of this geometry: only then are the planes it left in the context (smoothed,
// plane_s) the ones a call without a plane of its own means.
bool last_canny_was(const canny_hip_ctx *ctx, int n_frames, int height, int width)
{
    return ctx->last_canny_n && ctx->last_canny_n == n_frames && ctx->last_canny_h == height && ctx->last_canny_w == width;
}

size_t npx(int height, int width, int n_frames) { return (size_t)height * (size_t)width * (size_t)n_frames; }

// ---- colour input ---------------------------------------------------------------------------------
// A colour call's input as the kernels see it: bytes per pixel, the rule with its weights in the layout's byte order,
// and whether the Gaussian may convert.  Resolved once per call on the caller's context and handed to the batch
// pipelines' sub-contexts as it is (they do not share the caller's options).
struct ColorIn {
    int layout = CANNY_HIP_GRAY8;
    int ch = 1;
    GrayRule rule{};
    bool fuse = true;
};

int make_color_in(const canny_hip_ctx *ctx, int layout, ColorIn &ci)
{
    // (wb, wg, wr, shift): OpenCV's RGB2Gray<uchar> (B2Y / G2Y / R2Y, yuv_shift 14) and PIL's convert('L')
    static const uint32_t kRules[2][4] = {{1868u, 9617u, 4899u, 14u}, {7471u, 38470u, 19595u, 16u}};
    const uint32_t *w = kRules[ctx->gray_rule];
    ci.layout = layout;
    ci.fuse = ctx->fuse_gray != 0;
    switch (layout) {
    case CANNY_HIP_GRAY8: ci.ch = 1; break;
    case CANNY_HIP_BGR8: ci.ch = 3; break;
    case CANNY_HIP_RGB8: ci.ch = 3; break;
    case CANNY_HIP_BGRA8: ci.ch = 4; break;
    case CANNY_HIP_RGBA8: ci.ch = 4; break;
    default: return CANNY_HIP_ERR_INVALID;
    }
    const bool bgr = layout == CANNY_HIP_BGR8 || layout == CANNY_HIP_BGRA8;
    ci.rule.k0 = bgr ? w[0] : w[2];
    ci.rule.k1 = w[1];
    ci.rule.k2 = bgr ? w[2] : w[0];
    ci.rule.shift = w[3];
    ci.rule.rnd = 1u << (w[3] - 1);
    return CANNY_HIP_OK;
}

// ---- device-level stages ------------------------------------------------------------------------
// Can the Gaussian hand its result to Sobel+NMS as bytes?  (marching symmetric-tap kernel on both sides)
bool gaussian_u8_possible(const canny_hip_ctx *ctx, const GaussTaps &taps, int h, int w)
{
    float min_tap = 1.0f;
    for (int k = 0; k <= 2 * taps.center; k++)
        if (taps.tap[k] > 0.0f && taps.tap[k] < min_tap) min_tap = taps.tap[k];
    return ctx->gaussian_path != 1 && gaussian_march_supported(taps.center, h, w) && min_tap >= 0x1p-48f &&
           gaussian_march_u8_supported(taps) && sobel_nms_u8_input_supported();
}

// u8_mode: 0 = s16 plane in d_out; 1 = u8 plane in d_out, only if gaussian_u8_possible()
int dev_gaussian(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int h, int w, int n, void *d_out_any,
                 int u8_mode = 0)
{
    short *d_out = (short *)d_out_any;
    GaussTaps taps;
    int rc = make_taps(sigma, taps);
    if (rc) return rc;
    StageTimer tm(ctx, CANNY_HIP_STAGE_GAUSSIAN);
    if (u8_mode) {
        if (!gaussian_u8_possible(ctx, taps, h, w)) return CANNY_HIP_ERR_UNSUPPORTED;
        HIP_TRY(ctx, launch_gaussian_march_u8(d_img, (uint8_t *)d_out_any, h, w, n, taps, ctx->stream));
        return CANNY_HIP_OK;
    }
    // The marching kernel divides through a precomputed reciprocal, which equals the IEEE quotient for every
    // dividend >= 2^-102 (canny_hip_selftest_div).  Non-zero dividends are >= min_tap (row sums, pixels >= 1)
    // and >= ~min_tap^2 (column sums), so min_tap >= 2^-48 keeps them all above 2^-97; narrower taps
    // (sigma < ~0.13) take the generic kernels, which use the IEEE divide itself.
    float min_tap = 1.0f;
    for (int k = 0; k <= 2 * taps.center; k++)
        if (taps.tap[k] > 0.0f && taps.tap[k] < min_tap) min_tap = taps.tap[k];
    const bool can_march = gaussian_march_supported(taps.center, h, w) && min_tap >= 0x1p-48f;
    if (ctx->gaussian_path == 2 && !can_march) return CANNY_HIP_ERR_UNSUPPORTED;
    if (can_march && ctx->gaussian_path != 1) {
        HIP_TRY(ctx, launch_gaussian_march(d_img, d_out, h, w, n, taps, ctx->stream));
    } else {
        HIP_TRY(ctx, ctx->tmp_f32.ensure(npx(h, w, n) * sizeof(float)));
        HIP_TRY(ctx, launch_gaussian_generic(d_img, (float *)ctx->tmp_f32.p, d_out, h, w, n, taps, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// colour -> gray on the device (GRAY8: a copy, unless in place)
int dev_to_gray(canny_hip_ctx *ctx, const unsigned char *d_src, const ColorIn &ci, int h, int w, int n,
                unsigned char *d_gray)
{
    const size_t px = npx(h, w, n);
    if (ci.ch == 1) {
        if (d_src != d_gray) HIP_TRY(ctx, hipMemcpyAsync(d_gray, d_src, px, hipMemcpyDeviceToDevice, ctx->stream));
        return CANNY_HIP_OK;
    }
    StageTimer tm(ctx, CANNY_HIP_STAGE_TO_GRAY);
    HIP_TRY(ctx, launch_to_gray(d_src, ci.ch, ci.rule, d_gray, px, ctx->stream));
    return CANNY_HIP_OK;
}

// Can the Gaussian of canny()'s u8 path convert colour input itself?
bool gaussian_color_fusable(const canny_hip_ctx *ctx, const GaussTaps &taps, const ColorIn &ci, int h, int w)
{
    return ci.ch > 1 && gaussian_u8_possible(ctx, taps, h, w) && gaussian_march_color_supported(taps, w, ci.ch);
}

// The fused Gaussian alone: colour in, u8 smoothed plane out
int dev_gaussian_u8_color(canny_hip_ctx *ctx, const unsigned char *d_src, const ColorIn &ci, float sigma, int h, int w,
                          int n, unsigned char *d_out)
{
    GaussTaps taps;
    int rc = make_taps(sigma, taps);
    if (rc) return rc;
    if (!gaussian_color_fusable(ctx, taps, ci, h, w)) return CANNY_HIP_ERR_UNSUPPORTED;
    StageTimer tm(ctx, CANNY_HIP_STAGE_GAUSSIAN);
    HIP_TRY(ctx, launch_gaussian_march_u8_color(d_src, ci.ch, ci.rule, d_out, h, w, n, taps, ctx->stream));
    return CANNY_HIP_OK;
}

int ensure_hyst(canny_hip_ctx *ctx, const HystGeom &g)
{
    HIP_TRY(ctx, ctx->plane_s.ensure(g.words() * sizeof(uint64_t)));
    HIP_TRY(ctx, ctx->plane_c.ensure(g.words() * sizeof(uint64_t)));
    HIP_TRY(ctx, ctx->stamps.ensure((hyst_sched_words(g) + 4) * sizeof(unsigned))); // room for two lanes
    HIP_TRY(ctx, ctx->flags.ensure(4 * sizeof(unsigned)));
    if (!ctx->host_flags) {
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->host_flags, 8 * sizeof(unsigned), hipHostMallocMapped));
        std::memset(ctx->host_flags, 0, 8 * sizeof(unsigned));
        HIP_TRY(ctx, hipHostGetDevicePointer((void **)&ctx->host_flags_dev, ctx->host_flags, 0));
    }
    if (!ctx->flag_event) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->flag_event, hipEventDisableTiming));
    return CANNY_HIP_OK;
}

int ensure_aux_stream(canny_hip_ctx *ctx)
{
    if (!ctx->aux_stream) {
        // highest priority: what runs here is short and latency bound, and the main stream's kernels fill the chip
        int least = 0, greatest = 0;
        HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, greatest));
    }
    if (!ctx->fork_event) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming));
    if (!ctx->aux_event) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->aux_event, hipEventDisableTiming));
    return CANNY_HIP_OK;
}

// First launch of a hysteresis call: clears the scheduling words and the flags (flags[0] = last_change,
// flags[1] = domain) and, for planes filled by the Sobel+NMS kernel, the tile padding.
int prepare_hyst(canny_hip_ctx *ctx, const HystGeom &g, bool zero_pad)
{
    HIP_TRY(ctx, launch_hyst_prepare((uint64_t *)ctx->plane_s.p, (uint64_t *)ctx->plane_c.p, g, zero_pad,
                                     (unsigned *)ctx->stamps.p, (unsigned *)ctx->flags.p, ctx->stream));
    return CANNY_HIP_OK;
}

// Runs propagation sweeps until no tile was re-stamped, then (or meanwhile) the consumer of the strong plane.
// Sweeps are launched eight at a time before the host looks at the flag: natural images converge in 5-10
// sweeps, and a sweep with an empty queue costs ~4 us while a host round trip costs ~25 us.
// speculative: the consumer is a pure function of the strong plane that overwrites all of its output (the
// finalize kernel), so it is launched right behind each chunk of sweeps, BEFORE the host has seen the flag;
// the host waits on an event recorded behind the flag copy only, and the GPU never idles for the round trip.
// If the flag says "not converged" (rare) the consumer simply runs again behind the next chunk.
// edges != nullptr: the sweeps write the pixels they promote straight into that edge map (which must already
// hold the strong pixels); there is then nothing left for a consumer to do.
constexpr int kTailMaxTiles = 4096; // per frame (a 4K frame has 2040): beyond that one workgroup per frame is too few
constexpr int kSweepChunk = 8;
constexpr int kMaxSweeps = 1 << 22;

// Launches the next chunk of sweeps of a lane and, behind them, the one-thread kernel that publishes the two
// flag words and a sequence number in pinned host memory (the host spins on the sequence number: ~5 us from the
// last sweep to the host knowing, against ~35 us for an async copy plus an event wait).
int lane_launch_chunk(canny_hip_ctx *ctx, PropLane &L)
{
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_HYST_PROPAGATE, L.stream);
        for (int k = 0; k < kSweepChunk; k++)
            HIP_TRY(ctx, launch_hyst_propagate(L.S, L.C, L.sched, L.flags, L.iter + k, L.g, L.stream, L.edges,
                                               L.edge_value));
    }
    L.iter += kSweepChunk;
    L.seq = ++ctx->publish_seq;
    HIP_TRY(ctx, launch_hyst_publish(L.flags, L.host_dev, L.seq, L.stream));
    HIP_TRY(ctx, hipEventRecord(L.event, L.stream));
    return CANNY_HIP_OK;
}

// Waits for the chunk launched last and reads its verdict into L.converged.
int lane_wait(canny_hip_ctx *ctx, PropLane &L)
{
    volatile unsigned *hf = L.host;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (__atomic_load_n(&hf[2], __ATOMIC_ACQUIRE) != L.seq) {
        __builtin_ia32_pause();
        if ((++spins & 0xfffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIP_TRY(ctx, hipEventSynchronize(L.event)); // errors surface here
            if (__atomic_load_n(&hf[2], __ATOMIC_ACQUIRE) != L.seq) return CANNY_HIP_ERR_RUNTIME;
        }
    }
    if (hf[1]) return CANNY_HIP_ERR_DOMAIN;
    L.converged = hf[0] != (unsigned)L.iter; // nothing was scheduled for sweep `iter`
    if (!L.converged && L.iter >= kMaxSweeps) return CANNY_HIP_ERR_NO_CONVERGE;
    if (L.converged) ctx->last_hyst_iters = std::max(ctx->last_hyst_iters, (int)hf[0] + 1);
    return CANNY_HIP_OK;
}

// The whole frame range of a call as one lane on the context's stream.
PropLane main_lane(canny_hip_ctx *ctx, const HystGeom &g, short *edges, int edge_value)
{
    PropLane L;
    L.stream = ctx->stream;
    L.S = (uint64_t *)ctx->plane_s.p;
    L.C = (const uint64_t *)ctx->plane_c.p;
    L.sched = (unsigned *)ctx->stamps.p;
    L.flags = (unsigned *)ctx->flags.p;
    L.host = ctx->host_flags;
    L.host_dev = ctx->host_flags_dev;
    L.event = ctx->flag_event;
    L.g = g;
    L.edges = edges;
    L.edge_value = edge_value;
    return L;
}

template <class Consumer>
int run_propagation(canny_hip_ctx *ctx, const HystGeom &g, bool speculative, Consumer &&consumer,
                    short *edges = nullptr, int edge_value = 0)
{
    PropLane L = main_lane(ctx, g, edges, edge_value);
    ctx->last_hyst_iters = 0;
    ctx->hyst_iters_async = false;
    int rc;
    do {
        if ((rc = lane_launch_chunk(ctx, L))) return rc;
        if (speculative && (rc = consumer())) return rc;
        if ((rc = lane_wait(ctx, L))) return rc;
    } while (!L.converged);
    return speculative ? CANNY_HIP_OK : consumer();
}

// Second half of hysteresis, from filled bit-planes to the s16 edge map (every pixel of d_out is written).
int propagate_and_finalize(canny_hip_ctx *ctx, const HystGeom &g, short *d_out, int hi)
{
    return run_propagation(ctx, g, /*speculative=*/true, [&]() -> int {
        StageTimer tm(ctx, CANNY_HIP_STAGE_HYST_FINALIZE);
        // reached pixels hold EDGE=255 and survive the final `< max_val -> 0` sweep only if 255 >= max_val
        HIP_TRY(ctx, launch_hyst_finalize(d_out, (const uint64_t *)ctx->plane_s.p, g, 255 >= hi ? 255 : 0,
                                          ctx->stream));
        return CANNY_HIP_OK;
    });
}

int finish_pending(canny_hip_ctx *ctx);

// Per-frame thresholds of a dev_canny call (canny_hip_*_thresholds / _auto).  No spec = the call's (lo, hi) pair.
//   pairs:  device array of 2 * n ints, frame f's pair at [2f], [2f+1] (clamped into [1,255] by the kernels), or
//   rule:   an automatic rule (kAutoMedian / kAutoQuantile) with its parameters; the pairs it selects are written to
//           `out` (device, 2 * n ints), or to a context workspace if out is null.
struct ThrSpec {
    const int *pairs = nullptr;
    int rule = 0;
    double low = 0.0, high = 0.0;
    int *out = nullptr;
};

// Parameters of an automatic rule (section 1 of DESIGN.md section 11); finite values only.
bool auto_params_valid(int rule, float low, float high)
{
    if (!std::isfinite(low) || !std::isfinite(high)) return false;
    if (rule == kAutoMedian) return 0.0f <= low && low <= high;
    if (rule == kAutoQuantile) return 0.0f < low && low <= high && high <= 1.0f;
    return false;
}

// pairs != nullptr: per-frame thresholds, lo / hi ignored
int dev_hysteresis(canny_hip_ctx *ctx, short *d_cand, int h, int w, int n, int lo, int hi, const int *pairs = nullptr)
{
    if (pairs) lo = hi = 255; // (a clamped pair is in the domain: promoted pixels are 255)
    if (hysteresis_order_dependent(lo, hi)) return CANNY_HIP_ERR_DOMAIN;
    HystGeom g = make_hyst_geom(h, w, n);
    int rc = finish_pending(ctx); // a streamed call's sweeps own the planes until they are done
    if (rc || (rc = ensure_hyst(ctx, g))) return rc;
    if ((rc = prepare_hyst(ctx, g, /*zero_pad=*/false))) return rc; // the classify kernels write whole tiles
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_HYST_CLASSIFY);
        HIP_TRY(ctx, launch_hyst_classify(d_cand, (uint64_t *)ctx->plane_s.p, (uint64_t *)ctx->plane_c.p, g, lo, hi,
                                          (unsigned *)ctx->flags.p + 1, ctx->stream, pairs));
    }
    return propagate_and_finalize(ctx, g, d_cand, hi);
}

// Fused Sobel+NMS on a smoothed plane in [0,255].
int dev_sobel_nms(canny_hip_ctx *ctx, const short *d_smoothed, int h, int w, int n, short *d_out)
{
    if (ctx->sobel_nms_path != 1 && sobel_nms_march_supported(h, w)) {
        StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS, nullptr, /*attached=*/true);
        HIP_TRY(ctx, launch_sobel_nms_march(d_smoothed, d_out, h, w, n, ctx->stream, ctx->tune_sobel_seg,
                                            tm.launch_events()));
    } else {
        StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS);
        HIP_TRY(ctx, launch_sobel_nms(d_smoothed, d_out, h, w, n, /*domain8=*/true, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// color: interleaved colour input (canny_hip_*_color); null = the gray plane of every other entry point
// thr: per-frame thresholds (ThrSpec); null = (lo, hi) for every frame
int dev_canny(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
              short *d_edges, const ColorIn *color = nullptr, const ThrSpec *thr = nullptr)
{
    if (h < 2 || w < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    // per-frame pairs are clamped into [1,255]: the fused kernel takes every frame, promoted pixels are 255
    if (thr) lo = hi = 255;
    if (hysteresis_order_dependent(lo, hi)) return CANNY_HIP_ERR_DOMAIN;
    int rc = finish_pending(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, ctx->smoothed.ensure(npx(h, w, n) * sizeof(short)));
    short *sm = (short *)ctx->smoothed.p;
    const bool fused = ctx->fuse_classify && ctx->sobel_nms_path != 1 && sobel_nms_classify_supported(h, w, lo);
    int sm_u8 = 0; // the smoothed plane as bytes: only between the two marching kernels of the fused path
    if (fused && ctx->smoothed_u8) {
        GaussTaps taps;
        if ((rc = make_taps(sigma, taps))) return rc;
        if (gaussian_u8_possible(ctx, taps, h, w)) sm_u8 = ctx->smoothed_u8;
    }
    ctx->last_canny_u8 = sm_u8;
    ctx->last_canny_n = n, ctx->last_canny_h = h, ctx->last_canny_w = w;
    if (color && color->ch > 1) {
        // colour: the u8 Gaussian converts as it loads where it can, else a standalone pass converts first and the
        // gray path runs unchanged on the context's gray workspace
        GaussTaps taps;
        if ((rc = make_taps(sigma, taps))) return rc;
        const bool fuse = sm_u8 && color->fuse && gaussian_color_fusable(ctx, taps, *color, h, w);
        ctx->last_fused_gray = fuse;
        if (fuse) {
            StageTimer tm(ctx, CANNY_HIP_STAGE_GAUSSIAN);
            HIP_TRY(ctx, launch_gaussian_march_u8_color(d_img, color->ch, color->rule, (uint8_t *)sm, h, w, n, taps,
                                                        ctx->stream));
        } else {
            HIP_TRY(ctx, ctx->gray.ensure(npx(h, w, n)));
            if ((rc = dev_to_gray(ctx, d_img, *color, h, w, n, (unsigned char *)ctx->gray.p))) return rc;
            if ((rc = dev_gaussian(ctx, (const unsigned char *)ctx->gray.p, sigma, h, w, n, sm, sm_u8))) return rc;
        }
    } else {
        if (color) ctx->last_fused_gray = 0;
        if ((rc = dev_gaussian(ctx, d_img, sigma, h, w, n, sm, sm_u8))) return rc;
    }
    // per-frame thresholds: an automatic rule measures every frame's smoothed plane (median) or its gradient
    // magnitudes (quantile) and selects the pairs on the device; nothing comes back to the host
    const int *pairs = thr ? thr->pairs : nullptr;
    if (thr && thr->rule) {
        int *out = thr->out;
        if (!out) {
            HIP_TRY(ctx, ctx->thr.ensure((size_t)n * 2 * sizeof(int)));
            out = (int *)ctx->thr.p;
        }
        HIP_TRY(ctx, ctx->hist.ensure((size_t)n * kHistBins * sizeof(uint32_t)));
        uint32_t *hist = (uint32_t *)ctx->hist.p;
        StageTimer tm(ctx, CANNY_HIP_STAGE_HYST_CLASSIFY); // (no stage of its own: the thresholds are classify's input)
        HIP_TRY(ctx, hipMemsetAsync(hist, 0, (size_t)n * kHistBins * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, thr->rule == kAutoMedian ? launch_hist_intensity(sm, sm_u8 != 0, hist, h, w, n, ctx->stream)
                                              : launch_hist_gradient(sm, sm_u8 != 0, hist, h, w, n, ctx->stream));
        HIP_TRY(ctx, launch_thr_select(hist, n, thr->rule, thr->low, thr->high, out, ctx->stream));
        pairs = out;
    }
    // Sobel+NMS+classify on the s16 or the u8 smoothed plane
    auto fused_sobel = [&](const short *smp, short *edges, uint64_t *S, uint64_t *C, const HystGeom &gg, int ev,
                           const LaunchEvents &le, const int *pp) -> hipError_t {
        return sm_u8 ? launch_sobel_nms_classify_march_u8in((const uint8_t *)smp, edges, S, C, gg, lo, hi, ev,
                                                            ctx->stream, ctx->tune_sobel_seg, le, pp)
                     : launch_sobel_nms_classify_march(smp, edges, S, C, gg, lo, hi, ev, ctx->stream,
                                                       ctx->tune_sobel_seg, le, pp);
    };
    if (fused) {
        // Sobel+NMS writes the hysteresis bit-planes directly: the suppressed magnitudes never reach memory
        // and the classify pass disappears (canny() does not return them; the stage API still does).
        HystGeom g = make_hyst_geom(h, w, n);
        if ((rc = ensure_hyst(ctx, g))) return rc;
        uint64_t *S = (uint64_t *)ctx->plane_s.p, *C = (uint64_t *)ctx->plane_c.p;
        // reached pixels hold EDGE=255 and survive the reference's final `< max_val -> 0` sweep only if 255 >= max_val
        const int edge_value = 255 >= hi ? 255 : 0;
        if (ctx->overlap_hysteresis && n >= 16) {
            // Two halves.  The sweeps of half A run on a second stream while the main stream does Sobel+NMS of
            // half B: the sweeps are bound by launch and tile-load latency and leave most of the chip idle, the
            // Sobel+NMS kernel fills it.  Only half B's propagation remains exposed at the end of the call.
            if ((rc = ensure_aux_stream(ctx))) return rc;
            const int nA = n / 2, nB = n - nA;
            const HystGeom gA = make_hyst_geom(h, w, nA), gB = make_hyst_geom(h, w, nB);
            const size_t px_a = npx(h, w, nA);
            HIP_TRY(ctx, launch_hyst_prepare(S, C, g, /*zero_pad=*/true, (unsigned *)ctx->stamps.p,
                                             (unsigned *)ctx->flags.p, ctx->stream, /*n_lanes=*/2));
            PropLane A = main_lane(ctx, gA, d_edges, edge_value), B = main_lane(ctx, gB, d_edges + px_a, edge_value);
            A.stream = ctx->aux_stream;
            A.event = ctx->aux_event;
            B.S += gA.words();
            B.C += gA.words();
            B.sched += hyst_sched_words(gA);
            B.flags += 2;
            B.host += 4;
            B.host_dev += 4;
            {
                StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS, nullptr, /*attached=*/true);
                HIP_TRY(ctx, fused_sobel(sm, d_edges, A.S, (uint64_t *)A.C, gA, edge_value, tm.launch_events(), pairs));
            }
            HIP_TRY(ctx, hipEventRecord(ctx->fork_event, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->fork_event, 0));
            ctx->last_hyst_iters = 0;
            if ((rc = lane_launch_chunk(ctx, A))) return rc;
            {
                StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS, nullptr, /*attached=*/true);
                const short *smB = sm_u8 ? (const short *)((const uint8_t *)sm + px_a) : sm + px_a;
                HIP_TRY(ctx, fused_sobel(smB, d_edges + px_a, B.S, (uint64_t *)B.C, gB, edge_value, tm.launch_events(),
                                         pairs ? pairs + 2 * (size_t)nA : nullptr));
            }
            if ((rc = lane_launch_chunk(ctx, B))) return rc;
            for (PropLane *L : {&A, &B}) {
                if ((rc = lane_wait(ctx, *L))) return rc;
                while (!L->converged) {
                    if ((rc = lane_launch_chunk(ctx, *L)) || (rc = lane_wait(ctx, *L))) return rc;
                }
            }
            // whatever the caller queues on the context's stream next must see half A's edge map complete
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, A.event, 0));
            return CANNY_HIP_OK;
        }
        if ((rc = prepare_hyst(ctx, g, /*zero_pad=*/true))) return rc; // the kernel below writes in-image bytes only
        {
            StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS, nullptr, /*attached=*/true);
            HIP_TRY(ctx, fused_sobel(sm, d_edges, S, C, g, edge_value, tm.launch_events(), pairs));
        }
        // d_edges now holds the strong pixels; the sweeps add every pixel they promote: no finalize pass
        if (ctx->hyst_tail && g.tiles_x * g.tiles_y <= kTailMaxTiles) {
            // two batch-wide sweeps (all tiles; then the tiles those re-scheduled, from the per-frame queues), then one
            // workgroup per frame runs the rest to convergence: everything is queued, nothing is waited for
            StageTimer tm(ctx, CANNY_HIP_STAGE_HYST_PROPAGATE);
            unsigned *sched = (unsigned *)ctx->stamps.p, *flags = (unsigned *)ctx->flags.p;
            const int wide = ctx->hyst_tail_after;
            for (int k = 0; k < wide; k++)
                HIP_TRY(ctx, launch_hyst_propagate(S, C, sched, flags, k, g, ctx->stream, d_edges, edge_value,
                                                   /*frame_queues=*/true));
            HIP_TRY(ctx, launch_hyst_tail(S, C, sched, flags, wide, g, ctx->stream, d_edges, edge_value));
            ctx->hyst_iters_async = true;
            return CANNY_HIP_OK;
        }
        ctx->hyst_iters_async = false;
        return run_propagation(ctx, g, /*speculative=*/false, []() -> int { return CANNY_HIP_OK; }, d_edges, edge_value);
    }
    if ((rc = dev_sobel_nms(ctx, sm, h, w, n, d_edges))) return rc;
    return dev_hysteresis(ctx, d_edges, h, w, n, lo, hi, pairs);
}

// Completes the propagation canny_hip_dev_canny_stream left in flight and joins it into the context's stream.
int finish_pending(canny_hip_ctx *ctx)
{
    if (!ctx->has_pend) return CANNY_HIP_OK;
    ctx->has_pend = false; // also on errors: the lane is not resumable
    PropLane &L = ctx->pend;
    int rc;
    if ((rc = lane_wait(ctx, L))) return rc;
    while (!L.converged)
        if ((rc = lane_launch_chunk(ctx, L)) || (rc = lane_wait(ctx, L))) return rc;
    if (L.stream != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, L.event, 0));
    return CANNY_HIP_OK;
}

// canny() for a stream of batches (the reference's capture loop, src/main.cpp:120-137, with batches for frames).
// A plain call ends with a host round trip: the host learns whether the sweeps converged before it returns, and
// the GPU idles until the next call's first kernel arrives (~20 us per call; a third of the time of a single 4K
// frame).  Here the call returns with its chunk of sweeps queued, and the NEXT call first queues its Gaussian
// (which touches none of the hysteresis state) and only then looks at the flag:
//   stream:  ... S(i-1) | P(i-1) sweeps, publish | G(i) ............ | prepare, S(i) | P(i) sweeps, publish |
//   host:                  call i: enqueue G(i); read P(i-1)'s flag (already there, or soon); enqueue the rest
// If the flag says "not converged" (rare: more than 8 sweeps), further chunks simply run behind G(i).
// stream_overlap = 1 puts the sweeps on a second, high-priority stream instead, so that G(i) runs BESIDE P(i-1):
// the sweeps are latency bound and G is VALU bound, but sweep 0's waves take slots from G's 5 waves/SIMD, and a
// 128-frame batch gains nothing (G 1.20 -> 1.37 ms for 0.26 ms of hidden sweeps).
// The bit-planes, scheduling words and the smoothed plane stay single-buffered: everything that writes them is
// ordered behind P(i-1), and the Gaussian writes only the smoothed plane, which S(i-1) has finished reading.
int dev_canny_stream(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                     short *d_edges)
{
    if (h < 2 || w < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    if (hysteresis_order_dependent(lo, hi)) return CANNY_HIP_ERR_DOMAIN;
    if (!(ctx->fuse_classify && ctx->sobel_nms_path != 1 && sobel_nms_classify_supported(h, w, lo)) ||
        (ctx->hyst_tail && make_hyst_geom(h, w, n).tiles_x * make_hyst_geom(h, w, n).tiles_y <= kTailMaxTiles)) {
        // shapes the fused kernel does not take: plain call, nothing left in flight.  With the per-frame tail kernel
        // a plain call does not wait for anything either, so there is nothing to defer.
        int rc = finish_pending(ctx);
        return rc ? rc : dev_canny(ctx, d_img, sigma, lo, hi, h, w, n, d_edges);
    }
    HIP_TRY(ctx, ctx->smoothed.ensure(npx(h, w, n) * sizeof(short)));
    short *sm = (short *)ctx->smoothed.p;
    int sm_u8 = 0;
    if (ctx->smoothed_u8) {
        GaussTaps taps;
        int rt = make_taps(sigma, taps);
        if (rt) return rt;
        if (gaussian_u8_possible(ctx, taps, h, w)) sm_u8 = ctx->smoothed_u8;
    }
    ctx->last_canny_u8 = sm_u8;
    ctx->last_canny_n = n, ctx->last_canny_h = h, ctx->last_canny_w = w;
    int rc = dev_gaussian(ctx, d_img, sigma, h, w, n, sm, sm_u8);
    if (rc) return rc;
    if ((rc = finish_pending(ctx))) return rc; // host waits here while the Gaussian runs
    HystGeom g = make_hyst_geom(h, w, n);
    if ((rc = ensure_hyst(ctx, g)) || (ctx->stream_overlap && (rc = ensure_aux_stream(ctx)))) return rc;
    const int edge_value = 255 >= hi ? 255 : 0;
    if ((rc = prepare_hyst(ctx, g, /*zero_pad=*/true))) return rc;
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS, nullptr, /*attached=*/true);
        if (sm_u8)
            HIP_TRY(ctx, launch_sobel_nms_classify_march_u8in((const uint8_t *)sm, d_edges, (uint64_t *)ctx->plane_s.p,
                                                              (uint64_t *)ctx->plane_c.p, g, lo, hi, edge_value,
                                                              ctx->stream, ctx->tune_sobel_seg, tm.launch_events()));
        else
            HIP_TRY(ctx, launch_sobel_nms_classify_march(sm, d_edges, (uint64_t *)ctx->plane_s.p,
                                                         (uint64_t *)ctx->plane_c.p, g, lo, hi, edge_value, ctx->stream,
                                                         ctx->tune_sobel_seg, tm.launch_events()));
    }
    ctx->pend = main_lane(ctx, g, d_edges, edge_value);
    if (ctx->stream_overlap) {
        HIP_TRY(ctx, hipEventRecord(ctx->fork_event, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->fork_event, 0));
        ctx->pend.stream = ctx->aux_stream;
        ctx->pend.event = ctx->aux_event;
    }
    ctx->last_hyst_iters = 0;
    ctx->hyst_iters_async = false; // this lane reports through its host flags (finish_pending), not through flags[0]
    if ((rc = lane_launch_chunk(ctx, ctx->pend))) return rc;
    ctx->has_pend = true;
    return CANNY_HIP_OK;
}

int h2d(canny_hip_ctx *ctx, DevBuf &b, const void *src, size_t bytes)
{
    HIP_TRY(ctx, b.ensure(bytes));
    HIP_TRY(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return CANNY_HIP_OK;
}
int d2h_sync(canny_hip_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

// ---- edge point lists (canny_points.hip) ----------------------------------
// The source is the context's strong plane (strong != nullptr: hysteresis has converged in stream order) or a packed
// bit map.  count + scan: d_offsets[0..n] receives the CSR offsets; the per-row prefixes stay in ctx->points.
int dev_points_count(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g,
                     unsigned long long *d_offsets)
{
    const size_t rows = (size_t)g.n_frames * g.height;
    HIP_TRY(ctx, ctx->points.ensure(g.n_frames * sizeof(unsigned long long) + rows * sizeof(uint32_t)));
    unsigned long long *totals = (unsigned long long *)ctx->points.p;
    uint32_t *row_words = (uint32_t *)(totals + g.n_frames);
    StageTimer tm(ctx, CANNY_HIP_STAGE_COMPACT);
    HIP_TRY(ctx, launch_points_count(strong, bits, g, row_words, ctx->stream));
    HIP_TRY(ctx, launch_points_scan(row_words, totals, d_offsets, g.height, g.n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

// scatter, behind dev_points_count of the same source on the same stream
int dev_points_scatter(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g,
                       const unsigned long long *d_offsets, unsigned *d_points, unsigned long long capacity)
{
    if (!capacity) return CANNY_HIP_OK;
    const uint32_t *row_words = (const uint32_t *)((const unsigned long long *)ctx->points.p + g.n_frames);
    StageTimer tm(ctx, CANNY_HIP_STAGE_COMPACT);
    HIP_TRY(ctx, launch_points_scatter(strong, bits, g, row_words, d_offsets, d_points, capacity, ctx->stream));
    return CANNY_HIP_OK;
}

// The prologue of every "canny, then the stage on its map" call: dev_canny (unchanged) into d_edges, or into the edges16
// workspace when the caller passes none.  *strong_out receives the source of the finished map: the strong plane, or null
// when the map is empty by rule (max_val > 255: the reference zeroes every reached pixel, src/utils.cpp:336-340,
// although strong bits are set); what a stage stores for the empty map is the stage's business.
// Every route through dev_canny leaves the converged strong plane of the WHOLE batch in ctx->plane_s, in stream order
// (DESIGN.md section 12 goes through them), so the s16 map is never re-read.
int dev_canny_map(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                  short *d_edges, const uint64_t **strong_out)
{
    if (!d_edges) {
        HIP_TRY(ctx, ctx->edges16.ensure(npx(h, w, n) * sizeof(short)));
        d_edges = (short *)ctx->edges16.p;
    }
    const int rc = dev_canny(ctx, d_img, sigma, lo, hi, h, w, n, d_edges);
    if (rc) return rc;
    *strong_out = hi > 255 ? nullptr : (const uint64_t *)ctx->plane_s.p;
    return CANNY_HIP_OK;
}

// dev_canny_map, then count + scan of its map.  *strong_out receives the source for the scatter; when it is null the
// offsets have been zeroed.
int dev_canny_points_count(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w,
                           int n, short *d_edges, unsigned long long *d_offsets, const uint64_t **strong_out)
{
    int rc = dev_canny_map(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, strong_out);
    if (rc) return rc;
    if (!*strong_out) {
        HIP_TRY(ctx, hipMemsetAsync(d_offsets, 0, ((size_t)n + 1) * sizeof(unsigned long long), ctx->stream));
        return CANNY_HIP_OK;
    }
    return dev_points_count(ctx, *strong_out, nullptr, make_hyst_geom(h, w, n), d_offsets);
}

// ---- connected components (canny_components.hip) ---------------------------
struct CcOut {
    int *labels;
    unsigned char *kept;
    int *stats;
    unsigned long long capacity;
    unsigned long long *offsets;
};

// The labelling of one source (the context's strong plane or packed bits), queued on the context's stream.
int dev_components(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_area,
                   const CcOut &out)
{
    const size_t rows = (size_t)g.n_frames * g.height;
    int *parent = out.labels;
    if (!parent) {
        HIP_TRY(ctx, ctx->cc_parent.ensure(npx(g.height, g.width, g.n_frames) * sizeof(int)));
        parent = (int *)ctx->cc_parent.p;
    }
    HIP_TRY(ctx, ctx->cc_ws.ensure(g.n_frames * sizeof(unsigned long long) + rows * sizeof(uint32_t)));
    unsigned long long *totals = (unsigned long long *)ctx->cc_ws.p;
    uint32_t *row_words = (uint32_t *)(totals + g.n_frames);
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfComponents + CANNY_HIP_CC_PART_LINK);
        HIP_TRY(ctx, launch_cc_link(strong, bits, g, parent, ctx->stream));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfComponents + CANNY_HIP_CC_PART_RESOLVE);
        HIP_TRY(ctx, launch_cc_resolve(strong, bits, g, parent, ctx->stream));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfComponents + CANNY_HIP_CC_PART_NUMBER);
        HIP_TRY(ctx, launch_cc_count(strong, bits, g, parent, min_area, row_words, ctx->stream));
        HIP_TRY(ctx, launch_points_scan(row_words, totals, out.offsets, g.height, g.n_frames, ctx->stream));
        if (out.labels || out.kept || (out.stats && out.capacity))
            HIP_TRY(ctx, launch_cc_number(strong, bits, g, parent, min_area, row_words, out.offsets, out.stats,
                                          out.capacity, ctx->stream));
    }
    if (out.labels || out.kept) {
        StageTimer tm(ctx, canny_hip_ctx::kProfComponents + CANNY_HIP_CC_PART_WRITE);
        HIP_TRY(ctx, launch_cc_write(strong, bits, g, parent, out.labels, out.kept, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// dev_canny (unchanged), then the labelling of its map from the converged strong plane.  The result follows the MAP:
// max_val > 255 leaves no edge pixel (see dev_canny_map).
int dev_canny_components(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                         short *d_edges, int min_area, const CcOut &out)
{
    const uint64_t *strong;
    int rc = dev_canny_map(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, &strong);
    if (rc) return rc;
    if (!strong) {
        HIP_TRY(ctx, hipMemsetAsync(out.offsets, 0, ((size_t)n + 1) * sizeof(unsigned long long), ctx->stream));
        if (out.labels) HIP_TRY(ctx, hipMemsetAsync(out.labels, 0, npx(h, w, n) * sizeof(int), ctx->stream));
        if (out.kept) HIP_TRY(ctx, hipMemsetAsync(out.kept, 0, npx(h, w, n), ctx->stream));
        return CANNY_HIP_OK;
    }
    return dev_components(ctx, strong, nullptr, make_hyst_geom(h, w, n), min_area, out);
}

// ---- outer contour chains (canny_contours.hip) -----------------------------
struct CtOut {
    int *stats;
    unsigned long long capacity;
    unsigned long long *offsets, *chain_offsets;
    int *points;
    unsigned long long point_capacity;
    unsigned long long *point_offsets;
};

// the chain points of a frame are summed in 32 bits: a chain has at most 8 * area + 1 of them
int check_contour_dims(int height, int width, int n_frames)
{
    const int rc = check_dims(height, width, n_frames);
    if (rc) return rc;
    return (long long)height * width > kContourMaxPixels ? CANNY_HIP_ERR_UNSUPPORTED : CANNY_HIP_OK;
}

bool contour_args_ok(const CtOut &out)
{
    return out.offsets && out.point_offsets && (out.chain_offsets || !out.capacity) && (out.points || !out.point_capacity);
}

// The chains of one source (the context's strong plane or packed bits), queued on the context's stream: the labelling up
// to its scan, the two walks around the second scan, and the records last (launch_cc_number replaces the roots' entries).
int dev_contours(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_area,
                 const CtOut &out)
{
    const size_t rows = (size_t)g.n_frames * g.height;
    const size_t ws_bytes = g.n_frames * sizeof(unsigned long long) + rows * sizeof(uint32_t);
    HIP_TRY(ctx, ctx->cc_parent.ensure(npx(g.height, g.width, g.n_frames) * sizeof(int)));
    HIP_TRY(ctx, ctx->cc_ws.ensure(ws_bytes));
    HIP_TRY(ctx, ctx->ct_ws.ensure(ws_bytes));
    int *parent = (int *)ctx->cc_parent.p;
    unsigned long long *totals = (unsigned long long *)ctx->cc_ws.p, *point_totals = (unsigned long long *)ctx->ct_ws.p;
    uint32_t *row_words = (uint32_t *)(totals + g.n_frames), *row_points = (uint32_t *)(point_totals + g.n_frames);
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfContours + CANNY_HIP_CONTOUR_PART_LABEL);
        HIP_TRY(ctx, launch_cc_link(strong, bits, g, parent, ctx->stream));
        HIP_TRY(ctx, launch_cc_resolve(strong, bits, g, parent, ctx->stream));
        HIP_TRY(ctx, launch_cc_count(strong, bits, g, parent, min_area, row_words, ctx->stream));
        HIP_TRY(ctx, launch_points_scan(row_words, totals, out.offsets, g.height, g.n_frames, ctx->stream));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfContours + CANNY_HIP_CONTOUR_PART_COUNT);
        HIP_TRY(ctx, launch_ct_count(strong, bits, g, parent, min_area, row_words, out.offsets, out.chain_offsets,
                                     out.capacity, row_points, ctx->stream));
        HIP_TRY(ctx, launch_points_scan(row_points, point_totals, out.point_offsets, g.height, g.n_frames, ctx->stream));
        if (out.capacity)
            HIP_TRY(ctx, launch_ct_place(g, row_words, out.offsets, row_points, out.point_offsets, out.chain_offsets,
                                         out.capacity, ctx->stream));
    }
    if (out.capacity && out.point_capacity) {
        StageTimer tm(ctx, canny_hip_ctx::kProfContours + CANNY_HIP_CONTOUR_PART_WRITE);
        HIP_TRY(ctx, launch_ct_write(strong, bits, g, parent, min_area, row_words, out.offsets, out.chain_offsets,
                                     out.capacity, out.points, out.point_capacity, ctx->stream));
    }
    if (out.stats && out.capacity) {
        StageTimer tm(ctx, canny_hip_ctx::kProfContours + CANNY_HIP_CONTOUR_PART_STATS);
        HIP_TRY(ctx, launch_cc_number(strong, bits, g, parent, min_area, row_words, out.offsets, out.stats, out.capacity,
                                      ctx->stream));
    }
    return CANNY_HIP_OK;
}

// dev_canny (unchanged), then the chains of its map from the converged strong plane.  The result follows the MAP:
// max_val > 255 leaves no edge pixel (see dev_canny_map).
int dev_canny_contours(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                       short *d_edges, int min_area, const CtOut &out)
{
    const uint64_t *strong;
    int rc = dev_canny_map(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, &strong);
    if (rc) return rc;
    if (!strong) {
        const size_t off_bytes = ((size_t)n + 1) * sizeof(unsigned long long);
        HIP_TRY(ctx, hipMemsetAsync(out.offsets, 0, off_bytes, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(out.point_offsets, 0, off_bytes, ctx->stream));
        if (out.chain_offsets) HIP_TRY(ctx, hipMemsetAsync(out.chain_offsets, 0, sizeof(unsigned long long), ctx->stream));
        return CANNY_HIP_OK;
    }
    return dev_contours(ctx, strong, nullptr, make_hyst_geom(h, w, n), min_area, out);
}

// ---- edge curves (canny_curves.hip) ----------------------------------------
struct CvOut {
    int *records;
    unsigned long long capacity;
    unsigned long long *offsets, *chain_offsets;
    int *points;
    unsigned long long point_capacity;
    unsigned long long *point_offsets;
};

bool curve_args_ok(const CvOut &out)
{
    return out.offsets && out.point_offsets && (out.chain_offsets || !out.capacity) && (out.points || !out.point_capacity);
}

// The curves of one source (the context's strong plane or packed bits), queued on the context's stream: the count walks,
// the two scans, and -- when records were asked for -- the write walks.  The row sums and frame totals live in the two
// workspaces of the contour chains' scans; the count kernel writes every row's word before a scan reads it.
int dev_curves(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, int min_length,
               const CvOut &out)
{
    const size_t rows = (size_t)g.n_frames * g.height;
    const size_t ws_bytes = g.n_frames * sizeof(unsigned long long) + rows * sizeof(uint32_t);
    HIP_TRY(ctx, ctx->cc_ws.ensure(ws_bytes));
    HIP_TRY(ctx, ctx->ct_ws.ensure(ws_bytes));
    unsigned long long *totals = (unsigned long long *)ctx->cc_ws.p, *point_totals = (unsigned long long *)ctx->ct_ws.p;
    uint32_t *row_curves = (uint32_t *)(totals + g.n_frames), *row_points = (uint32_t *)(point_totals + g.n_frames);
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfCurves + CANNY_HIP_CURVE_PART_COUNT);
        HIP_TRY(ctx, launch_cv_count(strong, bits, g, min_length, row_curves, row_points, ctx->stream));
        HIP_TRY(ctx, launch_points_scan(row_curves, totals, out.offsets, g.height, g.n_frames, ctx->stream));
        HIP_TRY(ctx, launch_points_scan(row_points, point_totals, out.point_offsets, g.height, g.n_frames, ctx->stream));
    }
    if (out.capacity) {
        StageTimer tm(ctx, canny_hip_ctx::kProfCurves + CANNY_HIP_CURVE_PART_WRITE);
        HIP_TRY(ctx, launch_cv_write(strong, bits, g, min_length, row_curves, row_points, out.offsets, out.point_offsets,
                                     out.chain_offsets, out.capacity, out.records, out.points, out.point_capacity,
                                     ctx->stream));
    } else if (out.chain_offsets) {
        HIP_TRY(ctx, hipMemsetAsync(out.chain_offsets, 0, sizeof(unsigned long long), ctx->stream));
    }
    return CANNY_HIP_OK;
}

// dev_canny (unchanged), then the curves of its map from the converged strong plane.  The result follows the MAP:
// max_val > 255 leaves no edge pixel (see dev_canny_map).
int dev_canny_curves(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                     short *d_edges, int min_length, const CvOut &out)
{
    const uint64_t *strong;
    int rc = dev_canny_map(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, &strong);
    if (rc) return rc;
    if (!strong) {
        const size_t off_bytes = ((size_t)n + 1) * sizeof(unsigned long long);
        HIP_TRY(ctx, hipMemsetAsync(out.offsets, 0, off_bytes, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(out.point_offsets, 0, off_bytes, ctx->stream));
        if (out.chain_offsets) HIP_TRY(ctx, hipMemsetAsync(out.chain_offsets, 0, sizeof(unsigned long long), ctx->stream));
        return CANNY_HIP_OK;
    }
    return dev_curves(ctx, strong, nullptr, make_hyst_geom(h, w, n), min_length, out);
}

// ---- polygon approximation of the chains (canny_polygons.hip) --------------
struct PgOut {
    unsigned epsilon_q8, ratio_q16;
    unsigned long long *vertex_offsets;
    int *vertices;
    unsigned long long vertex_capacity;
    long long *measures;
};

bool polygon_args_ok(const PgOut &out)
{
    return out.vertex_offsets && (out.vertices || !out.vertex_capacity) && out.ratio_q16 < 65536u;
}

int check_polygon_dims(int height, int width)
{
    if (height < 1 || width < 1) return CANNY_HIP_ERR_INVALID;
    return height > kPolygonMaxSide || width > kPolygonMaxSide ? CANNY_HIP_ERR_UNSUPPORTED : CANNY_HIP_OK;
}

// The stage on stored chains, queued on the context's stream.  The launches depend on capacity and on which outputs were
// asked for; the number of records is read on the device.
int dev_polygons(canny_hip_ctx *ctx, const unsigned long long *offsets, int n_frames, unsigned long long capacity,
                 const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity, int width,
                 const PgOut &out)
{
    // one block: masks | block sums | flags
    const size_t masks_bytes = (size_t)capacity * sizeof(unsigned long long);
    const size_t sums_bytes = (size_t)polygons_scan_blocks(capacity) * sizeof(unsigned long long);
    HIP_TRY(ctx, ctx->pg_ws.ensure(masks_bytes + sums_bytes + (size_t)point_capacity + 16));
    unsigned long long *masks = (unsigned long long *)ctx->pg_ws.p;
    unsigned long long *sums = (unsigned long long *)((char *)ctx->pg_ws.p + masks_bytes);
    uint8_t *flags = (uint8_t *)ctx->pg_ws.p + masks_bytes + sums_bytes;
    const int part = canny_hip_ctx::kProfPolygons;
    {
        StageTimer tm(ctx, part + CANNY_HIP_POLYGON_PART_SIMPLIFY);
        HIP_TRY(ctx, launch_pg_simplify(offsets, n_frames, capacity, chain_offsets, points, point_capacity, width,
                                        out.epsilon_q8, out.ratio_q16, out.vertex_offsets, masks, flags, out.measures,
                                        ctx->stream));
    }
    if (capacity) {
        StageTimer tm(ctx, part + CANNY_HIP_POLYGON_PART_SCAN);
        HIP_TRY(ctx, launch_pg_scan(offsets, n_frames, capacity, out.vertex_offsets, sums, ctx->stream));
    }
    if (capacity && (out.vertex_capacity || out.measures)) {
        StageTimer tm(ctx, part + CANNY_HIP_POLYGON_PART_EMIT);
        HIP_TRY(ctx, launch_pg_emit(offsets, n_frames, capacity, chain_offsets, points, point_capacity, width,
                                    out.vertex_offsets, masks, flags, out.vertices, out.vertex_capacity, out.measures,
                                    ctx->stream));
    }
    return CANNY_HIP_OK;
}

// dev_canny_contours (unchanged), then the stage.  max_val > 255 leaves offsets all zero, so the stage finds no record.
int dev_canny_polygons(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                       short *d_edges, int min_area, const CtOut &ct, const PgOut &out)
{
    const int rc = dev_canny_contours(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, min_area, ct);
    if (rc) return rc;
    return dev_polygons(ctx, ct.offsets, n, ct.capacity, ct.chain_offsets, ct.points, ct.point_capacity, w, out);
}

// ---- contour shape measures (canny_shapes.hip) ------------------------------
struct ShOut {
    unsigned long long *hull_offsets;
    int *hull;
    unsigned long long hull_capacity;
    long long *measures;
};

bool shape_args_ok(const ShOut &out) { return out.hull_offsets && (out.hull || !out.hull_capacity); }

int check_shape_dims(int height, int width)
{
    if (height < 1 || width < 1) return CANNY_HIP_ERR_INVALID;
    return height > kShapeMaxSide || width > kShapeMaxSide ? CANNY_HIP_ERR_UNSUPPORTED : CANNY_HIP_OK;
}

// The stage on stored chains, queued on the context's stream.  The launches depend on capacity and on which outputs were
// asked for; the number of records is read on the device.
int dev_shapes(canny_hip_ctx *ctx, const unsigned long long *offsets, int n_frames, unsigned long long capacity,
               const unsigned long long *chain_offsets, const int *points, unsigned long long point_capacity, int width,
               const ShOut &out)
{
    // one block: column extremes | lists | hulls | block sums
    const size_t ints_bytes = (shapes_ws_ints(point_capacity) * sizeof(int) + 15) & ~(size_t)15;
    const size_t sums_bytes = (size_t)polygons_scan_blocks(capacity) * sizeof(unsigned long long);
    HIP_TRY(ctx, ctx->sh_ws.ensure(ints_bytes + sums_bytes + 16));
    int *ws = (int *)ctx->sh_ws.p;
    unsigned long long *sums = (unsigned long long *)((char *)ctx->sh_ws.p + ints_bytes);
    const int part = canny_hip_ctx::kProfShapes;
    {
        StageTimer tm(ctx, part + CANNY_HIP_SHAPE_PART_MEASURE);
        HIP_TRY(ctx, launch_sh_measure(offsets, n_frames, capacity, chain_offsets, points, point_capacity, width,
                                       out.hull_offsets, ws, out.measures, ctx->stream));
    }
    if (capacity) {
        StageTimer tm(ctx, part + CANNY_HIP_SHAPE_PART_SCAN);
        HIP_TRY(ctx, launch_pg_scan(offsets, n_frames, capacity, out.hull_offsets, sums, ctx->stream));
    }
    if (capacity && (out.hull_capacity || out.measures)) {
        StageTimer tm(ctx, part + CANNY_HIP_SHAPE_PART_EMIT);
        HIP_TRY(ctx, launch_sh_emit(offsets, n_frames, capacity, chain_offsets, point_capacity, width, out.hull_offsets, ws,
                                    out.hull, out.hull_capacity, out.measures, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// dev_canny_contours (unchanged), then the stage.  max_val > 255 leaves offsets all zero, so the stage finds no record.
int dev_canny_shapes(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                     short *d_edges, int min_area, const CtOut &ct, const ShOut &out)
{
    const int rc = dev_canny_contours(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, min_area, ct);
    if (rc) return rc;
    return dev_shapes(ctx, ct.offsets, n, ct.capacity, ct.chain_offsets, ct.points, ct.point_capacity, w, out);
}

// ---- Euclidean distance transform (canny_edt.hip) --------------------------
struct EdtOut {
    int *dist2;
    float *dist;
    int *nearest;
};

int check_edt_dims(int height, int width, int n_frames)
{
    const int rc = check_dims(height, width, n_frames);
    if (rc) return rc;
    // dist2 and the pixel indices are 32-bit
    if ((long long)height * width >= 0x80000000LL || (long long)height * height + (long long)width * width >= 0x80000000LL)
        return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// The transform of one source (the context's strong plane or packed bits), queued on the context's stream.
int dev_edt(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const EdtOut &out)
{
    const size_t padded = (size_t)g.n_frames * g.height * edt_pitch(g);
    HIP_TRY(ctx, ctx->edt_cols.ensure(padded * sizeof(uint16_t)));
    if (!out.dist2) HIP_TRY(ctx, ctx->edt_stack.ensure(padded * sizeof(uint32_t)));
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfEdt + CANNY_HIP_EDT_PART_ROWS);
        HIP_TRY(ctx, launch_edt_rows(strong, bits, g, (uint16_t *)ctx->edt_cols.p, ctx->stream));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfEdt + CANNY_HIP_EDT_PART_COLUMNS);
        HIP_TRY(ctx, launch_edt_columns(g, (uint16_t *)ctx->edt_cols.p, out.dist2 ? nullptr : (uint32_t *)ctx->edt_stack.p,
                                        out.dist2, out.dist, out.nearest, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// dev_canny (unchanged), then the transform of its map from the converged strong plane.  The result follows the MAP:
// max_val > 255 leaves no edge pixel (see dev_canny_map), so every plane takes its "no edge pixel" value.
int dev_canny_edt(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                  short *d_edges, const EdtOut &out)
{
    const uint64_t *strong;
    int rc = dev_canny_map(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, &strong);
    if (rc) return rc;
    if (!strong) {
        const size_t count = npx(h, w, n);
        if (out.dist2) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)out.dist2, CANNY_HIP_EDT_NONE, count, ctx->stream));
        if (out.dist) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)out.dist, 0x7F800000, count, ctx->stream)); // +inf
        if (out.nearest) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)out.nearest, -1, count, ctx->stream));
        return CANNY_HIP_OK;
    }
    return dev_edt(ctx, strong, nullptr, make_hyst_geom(h, w, n), out);
}

// ---- Hough lines (canny_hough.hip) -----------------------------------------
struct HoughOut {
    float *d_lines;
    int *d_votes;
    unsigned *d_bases;
    int *d_counts;
    int *d_accum;
};

bool hough_args_valid(float rho, float theta, float min_theta, float max_theta)
{
    return std::isfinite(rho) && std::isfinite(theta) && std::isfinite(min_theta) && std::isfinite(max_theta) &&
           rho > 0.0f && theta > 0.0f && min_theta >= 0.0f && min_theta < max_theta && max_theta <= (float)M_PI;
}

// The geometry of the rule, in double on the host.
int hough_geometry(int height, int width, float rho, float theta, float min_theta, float max_theta, int *numangle,
                   int *numrho)
{
    if (height < 1 || width < 1 || !hough_args_valid(rho, theta, min_theta, max_theta)) return CANNY_HIP_ERR_INVALID;
    double na = std::floor(((double)max_theta - (double)min_theta) / (double)theta) + 1.0;
    if (na > 1.0 && std::fabs(M_PI - (na - 1.0) * (double)theta) < (double)theta / 2) na -= 1.0;
    const double nr = std::nearbyint((2.0 * ((double)width + (double)height) + 1.0) / (double)rho); // half to even
    if (nr < 1.0 || (na + 2.0) * (nr + 2.0) > 2147483647.0) return CANNY_HIP_ERR_UNSUPPORTED; // bases are 32-bit
    *numangle = (int)na;
    *numrho = (int)nr;
    return CANNY_HIP_OK;
}

void hough_tables(float rho, float theta, float min_theta, int numangle, float *tab_cos, float *tab_sin)
{
    const float irho = 1.0f / rho;
    float ang = min_theta;
    for (int n = 0; n < numangle; n++) {
        tab_cos[n] = (float)(std::cos((double)ang) * (double)irho);
        tab_sin[n] = (float)(std::sin((double)ang) * (double)irho);
        ang = ang + theta;
    }
}

// No cell collects more votes than this: along the axis whose table entry is the larger one (at least 1 / (rho sqrt 2))
// a run of pixels that round to one r is at most rho * sqrt 2 + 1 long (+ 2 for the float roundings at its ends), and
// there are at most max(height, width) such runs.  The peak histogram has one bin per possible vote value.
int hough_hist_bins(int height, int width, float rho, double *bins)
{
    const double per_run = std::ceil(1.4143 * (double)rho) + 3.0;
    *bins = std::min((double)height * width, (double)std::max(height, width) * per_run) + 1.0;
    return *bins <= (double)(1 << 26) ? CANNY_HIP_OK : CANNY_HIP_ERR_UNSUPPORTED;
}

// Checks that need no device and write nothing; the geometry on success.
int hough_prepare(const canny_hip_ctx *ctx, int height, int width, float rho, float theta, int lines_max,
                  float min_theta, float max_theta, const HoughOut &out, HoughGeom &hg, int *lds_rows)
{
    if (!out.d_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    int rc = hough_geometry(height, width, rho, theta, min_theta, max_theta, &hg.numangle, &hg.numrho);
    if (rc) return rc;
    if (lines_max > kHoughMaxLines) return CANNY_HIP_ERR_UNSUPPORTED;
    double bins;
    if ((rc = hough_hist_bins(height, width, rho, &bins))) return rc;
    hg.rho = rho;
    hg.theta = theta;
    hg.min_theta = min_theta;
    // 48 KiB by default: two 1024-lane workgroups per CU; a row of a 4K frame at rho 1 is 46.9 KiB
    const int fit = hough_lds_rows(hg, ctx->hough_lds_kb ? ctx->hough_lds_kb * 1024 : 48 * 1024);
    if (ctx->hough_path == 2 && !fit) return CANNY_HIP_ERR_UNSUPPORTED; // a row does not fit in LDS
    *lds_rows = ctx->hough_path == 1 ? 0 : fit;
    return CANNY_HIP_OK;
}

// The vote tables of hg on the device (ctx->hough_tab): they travel once per set of arguments; the host copy outlives its
// transfer.
int hough_tab_ensure(canny_hip_ctx *ctx, const HoughGeom &hg)
{
    const size_t tab_bytes = 2 * (size_t)hg.numangle * sizeof(float);
    const bool tab_moved = ctx->hough_tab.bytes < tab_bytes;
    HIP_TRY(ctx, ctx->hough_tab.ensure(tab_bytes));
    if (tab_moved || ctx->hough_tab_n != hg.numangle || ctx->hough_tab_key[0] != hg.rho ||
        ctx->hough_tab_key[1] != hg.theta || ctx->hough_tab_key[2] != hg.min_theta) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // an earlier transfer may still read the host copy
        ctx->hough_tab_host.resize(2 * (size_t)hg.numangle);
        hough_tables(hg.rho, hg.theta, hg.min_theta, hg.numangle, ctx->hough_tab_host.data(),
                     ctx->hough_tab_host.data() + hg.numangle);
        ctx->hough_tab_n = 0;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hough_tab.p, ctx->hough_tab_host.data(), tab_bytes, hipMemcpyHostToDevice,
                                    ctx->stream));
        ctx->hough_tab_n = hg.numangle;
        ctx->hough_tab_key[0] = hg.rho, ctx->hough_tab_key[1] = hg.theta, ctx->hough_tab_key[2] = hg.min_theta;
    }
    return CANNY_HIP_OK;
}

// The transform of one source (CSR points, packed bits or the context's strong plane), queued on the context's stream.
// All three null: the empty map (counts 0, a zero accumulator if the caller asked for it).
int dev_hough(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const unsigned *points,
              const unsigned long long *offsets, const HystGeom &g, const HoughGeom &hg, int lds_rows, int threshold,
              int lines_max, const HoughOut &out)
{
    const int n = g.n_frames;
    HIP_TRY(ctx, hipMemsetAsync(out.d_counts, 0, (size_t)n * sizeof(int), ctx->stream));
    if (!strong && !bits && !points) {
        if (out.d_accum) HIP_TRY(ctx, hipMemsetAsync(out.d_accum, 0, hough_accum_bytes(hg, n), ctx->stream));
        return CANNY_HIP_OK;
    }
    int *accum = out.d_accum;
    if (!accum) {
        HIP_TRY(ctx, ctx->hough_accum.ensure(hough_accum_bytes(hg, n)));
        accum = (int *)ctx->hough_accum.p;
    }
    int rc = hough_tab_ensure(ctx, hg);
    if (rc) return rc;
    double bins_d;
    (void)hough_hist_bins(g.height, g.width, hg.rho, &bins_d);
    const int bins = (int)bins_d;
    // workspace: candidate keys | histograms | tie counts per accumulator row | cut words
    const size_t cand_bytes = (size_t)n * lines_max * sizeof(unsigned long long);
    const size_t hist_bytes = (size_t)n * bins * sizeof(unsigned), ties_bytes = (size_t)n * hg.numangle * sizeof(unsigned);
    HIP_TRY(ctx, ctx->hough_ws.ensure(cand_bytes + hist_bytes + ties_bytes + (size_t)n * 8 * sizeof(unsigned)));
    unsigned long long *cand = (unsigned long long *)ctx->hough_ws.p;
    unsigned *hist = (unsigned *)((char *)ctx->hough_ws.p + cand_bytes);
    unsigned *ties = hist + (size_t)n * bins, *cut = ties + (size_t)n * hg.numangle;
    HIP_TRY(ctx, hipMemsetAsync(hist, 0, hist_bytes + ties_bytes, ctx->stream));
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_END + 0);
        HIP_TRY(ctx, launch_hough_vote(strong, bits, points, offsets, g, hg, (const float *)ctx->hough_tab.p, accum,
                                       lds_rows, ctx->stream));
    }
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_END + 1);
        HIP_TRY(ctx, launch_hough_peaks(accum, n, hg, threshold, out.d_counts, hist, bins, ctx->stream));
    }
    if (out.d_lines || out.d_votes || out.d_bases) {
        StageTimer tm(ctx, CANNY_HIP_STAGE_END + 2);
        HIP_TRY(ctx, launch_hough_select(accum, n, hg, threshold, lines_max, out.d_counts, hist, bins, ties, cut, cand,
                                         out.d_lines, out.d_votes, out.d_bases, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// ---- Hough circles (canny_hough_circles.hip) --------------------------------
struct CircleArgs {
    int min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max;
};
struct CircleOut {
    int *d_circles, *d_counts, *d_centre_counts, *d_accum;
};

// No cell collects more votes than this: the samples of a ray are |step| / 1024 >= 0.9993 pixels
// apart, so at most ceil(c sqrt 2) + 1 of them (and never more than there are radii) fall into one c x c cell; a pixel has
// two rays; a sample lies less than max_radius + 1 pixels from its pixel, so only the pixels of the cell grown by that much on
// every side, clipped to the frame, reach it.  The peak histogram has one bin per possible vote value.
int circles_hist_bins(int height, int width, const CircleGeom &cg, double *bins)
{
    const double c = (double)(1 << cg.cell_shift);
    const double per_ray = std::min((double)(cg.max_radius - cg.min_radius + 1), std::ceil(1.4143 * c) + 1.0);
    const double reach = c + 2.0 * ((double)cg.max_radius + 1.0);
    *bins = std::min((double)width, reach) * std::min((double)height, reach) * 2.0 * per_ray + 1.0;
    return *bins <= (double)(1 << 26) ? CANNY_HIP_OK : CANNY_HIP_ERR_UNSUPPORTED;
}

// Checks that need no device and write nothing; the geometry on success.
int circles_prepare(int height, int width, const CircleArgs &a, const int *counts, CircleGeom &cg)
{
    if (!counts || a.min_radius < 1 || a.min_radius > a.max_radius || a.cell_shift < 0 || a.cell_shift > 3 ||
        a.centres_max < 1 || a.min_dist < 0 || height < 2 || width < 2)
        return CANNY_HIP_ERR_INVALID;
    if (a.max_radius > kCircleMaxRadius || a.centres_max > kHoughMaxLines) return CANNY_HIP_ERR_UNSUPPORTED;
    const int c = 1 << a.cell_shift;
    cg.min_radius = a.min_radius, cg.max_radius = a.max_radius, cg.cell_shift = a.cell_shift;
    cg.aw = (width + c - 1) / c;
    cg.ah = (height + c - 1) / c;
    if (((double)cg.ah + 2.0) * ((double)cg.aw + 2.0) > 2147483647.0) return CANNY_HIP_ERR_UNSUPPORTED; // bases are 32-bit
    double bins;
    return circles_hist_bins(height, width, cg, &bins);
}

// THE step of the rule on the host (built with -ffp-contract=off): conversion, root and quotient each round once.
void circles_step_of(int gx, int gy, int *sx, int *sy)
{
    const unsigned q = (unsigned)(gx * gx) + (unsigned)(gy * gy);
    if (!q) {
        *sx = *sy = 0;
        return;
    }
    const float m = std::sqrt((float)q);
    const float qx = (float)(gx * 1024) / m, qy = (float)(gy * 1024) / m;
    *sx = (int)std::nearbyint(qx); // half to even (the default rounding mode)
    *sy = (int)std::nearbyint(qy);
}

// The transform of one source (packed bits with gradient planes, or the context's strong plane with its smoothed plane),
// queued on the context's stream.  Both sources null: the empty map (counts 0, a zero accumulator if the caller asked).
int dev_circles(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const void *smoothed,
                bool smoothed_u8, const short *d_gx, const short *d_gy, const CircleGeom &cg, const CircleArgs &a,
                const CircleOut &out)
{
    const int n = g.n_frames, cm = a.centres_max;
    HIP_TRY(ctx, hipMemsetAsync(out.d_counts, 0, (size_t)n * sizeof(int), ctx->stream));
    if (out.d_centre_counts) HIP_TRY(ctx, hipMemsetAsync(out.d_centre_counts, 0, (size_t)n * sizeof(int), ctx->stream));
    if (!strong && !bits) {
        if (out.d_accum) HIP_TRY(ctx, hipMemsetAsync(out.d_accum, 0, circles_accum_bytes(cg, n), ctx->stream));
        return CANNY_HIP_OK;
    }
    int *accum = out.d_accum;
    if (!accum) {
        HIP_TRY(ctx, ctx->circ_accum.ensure(circles_accum_bytes(cg, n)));
        accum = (int *)ctx->circ_accum.p;
    }
    double bins_d;
    (void)circles_hist_bins(g.height, g.width, cg, &bins_d);
    const int bins = (int)bins_d;
    // workspace: candidate keys | votes | bases | radii | supports | cut words | peak counts | histograms | tie counts per
    // accumulator row (the last three are zeroed together)
    const size_t slots = (size_t)n * cm;
    const size_t zero_words = (size_t)n + (size_t)n * bins + (size_t)n * cg.ah;
    HIP_TRY(ctx, ctx->circ_ws.ensure(slots * 8 + slots * 16 + ((size_t)n * 8 + zero_words) * sizeof(unsigned)));
    unsigned long long *cand = (unsigned long long *)ctx->circ_ws.p;
    int *votes = (int *)(cand + slots);
    unsigned *bases = (unsigned *)(votes + slots);
    int *radius = (int *)(bases + slots), *support = radius + slots;
    unsigned *cut = (unsigned *)(support + slots);
    int *peaks = (int *)(cut + (size_t)n * 8);
    unsigned *hist = (unsigned *)(peaks + n), *ties = hist + (size_t)n * bins;
    HIP_TRY(ctx, hipMemsetAsync(peaks, 0, zero_words * sizeof(unsigned), ctx->stream));
    if (out.d_centre_counts) peaks = out.d_centre_counts; // zeroed above
    const HoughGeom hg{cg.ah, cg.aw, 1.0f, 1.0f, 0.0f};   // the accumulator read as ah rows of aw cells
    const int part = canny_hip_ctx::kProfCircles;
    {
        StageTimer tm(ctx, part + CANNY_HIP_CIRCLE_PART_VOTE);
        HIP_TRY(ctx, launch_circles_vote(strong, bits, g, smoothed, smoothed_u8, d_gx, d_gy, cg, accum, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_CIRCLE_PART_CENTRES);
        HIP_TRY(ctx, launch_hough_peaks(accum, n, hg, a.threshold, peaks, hist, bins, ctx->stream));
        HIP_TRY(ctx, launch_hough_select(accum, n, hg, a.threshold, cm, peaks, hist, bins, ties, cut, cand, nullptr, votes,
                                         bases, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_CIRCLE_PART_RADIUS);
        HIP_TRY(ctx, launch_circles_radius(strong, bits, g, cg, bases, peaks, cm, radius, support, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_CIRCLE_PART_ACCEPT);
        HIP_TRY(ctx, launch_circles_accept(g, cg, bases, votes, radius, support, peaks, cm, a.support_threshold, a.min_dist,
                                           out.d_circles, out.d_counts, ctx->stream));
    }
    return CANNY_HIP_OK;
}

// ---- Hough line segments (canny_hough_segments.hip) ---------------------
struct SegArgs {
    int min_length, max_gap, exclusive, segments_max;
};

// THE check of the segment arguments; needs no device and writes nothing.  lines: the longest line list of a frame;
// on_device: the kernels' limit on exclusive mode applies (the host walk has none).
int segments_check(int height, int width, int n_frames, int lines, const SegArgs &a, bool on_device)
{
    if (a.min_length < 0 || a.max_gap < 0 || (a.exclusive != 0 && a.exclusive != 1) || a.segments_max < 1)
        return CANNY_HIP_ERR_INVALID;
    if ((double)n_frames * (double)a.segments_max * CANNY_HIP_SEGMENT_INTS >= 2147483648.0) return CANNY_HIP_ERR_UNSUPPORTED;
    // a line has at most ceil(L / 2) segments; a frame's count is an int
    if ((double)lines * (((double)std::max(height, width) + 1.0) / 2.0) >= 2147483648.0) return CANNY_HIP_ERR_UNSUPPORTED;
    // exclusive mode keeps one bit per major position in LDS
    if (on_device && a.exclusive && std::max(height, width) > kSegExclusiveMaxAxis) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// The rule's vote on the host (built with -ffp-contract=off: three roundings), for canny_hip_hough_segments_from_bits.
inline int host_vote_r(int x, int y, float c, float s, int half)
{
    const float a = (float)x * c, b = (float)y * s;
    return (int)std::nearbyintf(a + b) + half;
}

// The segments of one source (packed bits or the context's strong plane) along the lines in d_bases / d_line_counts,
// queued on the context's stream.  Both sources null: the empty map (all counts 0).
int dev_segments(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const HoughGeom &hg,
                 const unsigned *d_bases, const int *d_line_counts, int lines_max, const SegArgs &a, int *d_segments,
                 int *d_seg_counts)
{
    const int n = g.n_frames;
    if (!strong && !bits) {
        HIP_TRY(ctx, hipMemsetAsync(d_seg_counts, 0, (size_t)n * sizeof(int), ctx->stream));
        return CANNY_HIP_OK;
    }
    int rc = hough_tab_ensure(ctx, hg);
    if (rc) return rc;
    const float *tab = (const float *)ctx->hough_tab.p;
    const SegGeom sg{hg.numangle, hg.numrho, hough_segments_halfwin(g.height, g.width, hg.rho), a.min_length, a.max_gap,
                     lines_max, a.segments_max};
    const int part = canny_hip_ctx::kProfSegments;
    if (a.exclusive) {
        // The private copy is read and cleared as 32-bit words by one workgroup per frame with workgroup-scope atomics, so
        // no word may belong to two frames.  The plane's frames are whole 64-bit words already; packed bytes get a stride
        // of their own per frame (hough_segments_work_stride: a multiple of 128 bytes), whatever height * row bytes is.
        const size_t frame_bytes = bits ? (size_t)g.height * ((g.width + 7) / 8) : g.words() / n * sizeof(uint64_t);
        const size_t stride = bits ? hough_segments_work_stride(g) : frame_bytes;
        HIP_TRY(ctx, ctx->seg_work.ensure(stride * n));
        StageTimer tm(ctx, part + CANNY_HIP_SEGMENT_PART_EXCLUSIVE);
        if (bits)
            HIP_TRY(ctx, hipMemcpy2DAsync(ctx->seg_work.p, stride, bits, frame_bytes, frame_bytes, (size_t)n,
                                          hipMemcpyDeviceToDevice, ctx->stream));
        else
            HIP_TRY(ctx, hipMemcpyAsync(ctx->seg_work.p, strong, frame_bytes * n, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, launch_hough_segments_exclusive((uint32_t *)ctx->seg_work.p, bits != nullptr, g, sg, tab, d_bases,
                                                     d_line_counts, d_segments, d_seg_counts, ctx->stream));
        return CANNY_HIP_OK;
    }
    // per-line segment counts | their exclusive prefix within the frame
    const size_t slots = (size_t)n * lines_max;
    HIP_TRY(ctx, ctx->seg_ws.ensure(2 * slots * sizeof(int)));
    int *nseg = (int *)ctx->seg_ws.p, *line_off = nseg + slots;
    {
        StageTimer tm(ctx, part + CANNY_HIP_SEGMENT_PART_COUNT);
        HIP_TRY(ctx, launch_hough_segments_count(strong, bits, g, sg, tab, d_bases, d_line_counts, nseg, line_off,
                                                 d_seg_counts, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_SEGMENT_PART_EMIT);
        HIP_TRY(ctx, launch_hough_segments_emit(strong, bits, g, sg, tab, d_bases, d_line_counts, line_off, d_segments,
                                                ctx->stream));
    }
    return CANNY_HIP_OK;
}

void destroy_batch_pipe(canny_hip_ctx::BatchPipe *w)
{
    if (!w) return;
    if (w->sub) (void)hipSetDevice(w->sub->device);
    if (w->s_h2d) (void)hipStreamSynchronize(w->s_h2d);
    if (w->s_d2h) (void)hipStreamSynchronize(w->s_d2h);
    for (auto &sl : w->slot) {
        sl.d_in.release();
        sl.d_out.release();
        sl.d_out8.release();
        sl.pin_in.release();
        sl.pin_out.release();
        sl.d_thr.release();
        sl.pin_thr.release();
        for (hipEvent_t e : {sl.ev_h2d, sl.ev_comp, sl.ev_d2h})
            if (e) (void)hipEventDestroy(e);
    }
    if (w->s_h2d) (void)hipStreamDestroy(w->s_h2d);
    if (w->s_d2h) (void)hipStreamDestroy(w->s_d2h);
    if (w->owns_sub) canny_hip_ctx_destroy(w->sub);
    delete w;
}

int create_batch_pipe(canny_hip_ctx *ctx, bool first, canny_hip_ctx::BatchPipe **out)
{
    auto *w = new (std::nothrow) canny_hip_ctx::BatchPipe();
    if (!w) return CANNY_HIP_ERR_RUNTIME;
    int st = CANNY_HIP_OK;
    if (first) {
        w->sub = ctx;
    } else {
        st = canny_hip_ctx_create(&w->sub, ctx->device);
        w->owns_sub = st == CANNY_HIP_OK;
    }
    hipError_t e = hipSuccess;
    if (!st) {
        for (auto &sl : w->slot)
            for (hipEvent_t *ev : {&sl.ev_h2d, &sl.ev_comp, &sl.ev_d2h})
                if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) st = fail(ctx, e, "batch pipeline events");
    }
    if (st) {
        destroy_batch_pipe(w);
        return st;
    }
    *out = w;
    return CANNY_HIP_OK;
}

// the copy streams of three-stream mode
int ensure_copy_streams(canny_hip_ctx *ctx, canny_hip_ctx::BatchPipe &w)
{
    if (!w.s_h2d) HIP_TRY(ctx, hipStreamCreateWithFlags(&w.s_h2d, hipStreamNonBlocking));
    if (!w.s_d2h) HIP_TRY(ctx, hipStreamCreateWithFlags(&w.s_d2h, hipStreamNonBlocking));
    return CANNY_HIP_OK;
}

// Every device workspace of a context, for canny_hip_selftest_workspace: the rows of kWorkspaces (DESIGN.md section 20 has
// a row for each), the staging blocks io[4], then the staging of the cached batch pipelines and the
// workspaces of the sub-contexts they own.  Pipeline 0 computes on the context itself, so only its staging is new.
struct WsEntry {
    std::string name;
    const DevBuf *buf;
    int kind;
};

void collect_workspaces(const canny_hip_ctx *c, const std::string &prefix, std::vector<WsEntry> &v)
{
    const int D = CANNY_HIP_WS_DATA, I = CANNY_HIP_WS_INDEX;
    auto add = [&](const char *name, const DevBuf &b, int kind) { v.push_back({prefix + name, &b, kind}); };
    for (const WsRow &r : kWorkspaces) add(r.name, c->*r.buf, r.kind);
    for (int k = 0; k < 4; k++) add(("io" + std::to_string(k)).c_str(), c->io[k], I); // whatever a stage call staged last
    for (size_t p = 0; p < c->batch_pool.size(); p++) {
        const canny_hip_ctx::BatchPipe *w = c->batch_pool[p];
        if (!w) continue;
        const std::string pipe = prefix + "pipe" + std::to_string(p) + ".";
        for (int s = 0; s < canny_hip_ctx::BatchPipe::kSlots; s++) {
            const std::string slot = pipe + "slot" + std::to_string(s) + ".";
            v.push_back({slot + "d_in", &w->slot[s].d_in, D});
            v.push_back({slot + "d_out", &w->slot[s].d_out, D});
            v.push_back({slot + "d_out8", &w->slot[s].d_out8, D});
            v.push_back({slot + "d_thr", &w->slot[s].d_thr, D});
        }
        if (w->owns_sub && w->sub) collect_workspaces(w->sub, pipe, v);
    }
}

} // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int canny_hip_version(void) { return CANNY_HIP_VERSION; }

const char *canny_hip_status_string(int status)
{
    switch (status) {
    case CANNY_HIP_OK: return "ok";
    case CANNY_HIP_ERR_INVALID: return "invalid argument";
    case CANNY_HIP_ERR_UNSUPPORTED: return "unsupported size or window";
    case CANNY_HIP_ERR_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
    case CANNY_HIP_ERR_RUNTIME: return "HIP runtime error";
    case CANNY_HIP_ERR_DOMAIN: return "input outside the documented numeric domain";
    case CANNY_HIP_ERR_NO_CONVERGE: return "hysteresis propagation did not converge";
    default: return "unknown status";
    }
}

int canny_hip_device_count(int *count)
{
    if (!count) return CANNY_HIP_ERR_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return CANNY_HIP_ERR_NO_DEVICE;
    }
    *count = n;
    return CANNY_HIP_OK;
}

int canny_hip_ctx_create(canny_hip_ctx **out, int device)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        return CANNY_HIP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return CANNY_HIP_ERR_INVALID;
    canny_hip_ctx *ctx = new (std::nothrow) canny_hip_ctx();
    if (!ctx) return CANNY_HIP_ERR_RUNTIME;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        delete ctx;
        return CANNY_HIP_ERR_NO_DEVICE;
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return CANNY_HIP_OK;
}

void canny_hip_ctx_destroy(canny_hip_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)finish_pending(ctx);
    ctx->expand_pool.reset(); // joins its threads; no job can be queued here (batch calls are synchronous)
    for (auto *w : ctx->batch_pool) destroy_batch_pipe(w);
    ctx->batch_pool.clear();
    (void)hipSetDevice(ctx->device);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    (void)hipStreamSynchronize(ctx->stream);
    while (!ctx->chamfer_sets.empty()) (void)canny_hip_chamfer_set_destroy(ctx, ctx->chamfer_sets.back());
    for (const WsRow &r : kWorkspaces) (ctx->*r.buf).release();
    for (auto &b : ctx->io) b.release();
    if (ctx->host_flags) (void)hipHostFree(ctx->host_flags);
    if (ctx->flag_event) (void)hipEventDestroy(ctx->flag_event);
    if (ctx->fork_event) (void)hipEventDestroy(ctx->fork_event);
    if (ctx->aux_event) (void)hipEventDestroy(ctx->aux_event);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    for (auto &v : ctx->pending)
        for (auto &e : v) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
    for (auto &e : ctx->pool) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int canny_hip_ctx_set_stream(canny_hip_ctx *ctx, void *hip_stream)
{
    int rc = bind(ctx);
    if (rc || (rc = finish_pending(ctx))) return rc; // joins the old stream
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return CANNY_HIP_OK;
}

int canny_hip_ctx_device(const canny_hip_ctx *ctx) { return ctx ? ctx->device : -1; }

int canny_hip_ctx_get_option(const canny_hip_ctx *ctx, const char *name, int *value)
{
    if (!ctx || !name || !value) return CANNY_HIP_ERR_INVALID;
    for (const OptRow &o : kOptions)
        if (!std::strcmp(name, o.name)) {
            if (!o.readable) return CANNY_HIP_ERR_INVALID;
            *value = ctx->*o.field;
            return CANNY_HIP_OK;
        }
    if (!std::strcmp(name, "batch_expand_threads")) *value = ctx->expand_pool ? ctx->expand_pool->size() : 0; // read-only
    else return CANNY_HIP_ERR_INVALID;
    return CANNY_HIP_OK;
}

int canny_hip_ctx_set_option(canny_hip_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name || value < 0) return CANNY_HIP_ERR_INVALID;
    for (const OptRow &o : kOptions)
        if (!std::strcmp(name, o.name)) {
            if (!o.writable || value < o.min || value > o.max) return CANNY_HIP_ERR_INVALID;
            ctx->*o.field = value;
            return CANNY_HIP_OK;
        }
    if (!std::strcmp(name, "tune_batch_expand_threads") && value <= 64) {
        if (value != ctx->batch_expand_threads) ctx->expand_pool.reset();
        ctx->batch_expand_threads = value;
    }
    else if (!std::strcmp(name, "stream_overlap") && value <= 1) {
        int rc = bind(ctx);
        if (rc || (rc = finish_pending(ctx))) return rc;
        ctx->stream_overlap = value;
    } else if (!std::strcmp(name, "profile_sample_interval") && value >= 1) {
        ctx->prof_every = (unsigned)value;
        for (auto &n : ctx->prof_seen) n = 0;
    } else if (!std::strcmp(name, "profile_stage_mask")) ctx->prof_mask = value ? (unsigned)value : ~0u;
    else if (!std::strcmp(name, "tune_sobel_px") && value <= 1) sobel_nms_set_px_variant(value); // process-wide
    else if (!std::strcmp(name, "tune_sobel_variant") && value <= 2) sobel_nms_set_arith_variant(value); // process-wide
    else if (!std::strcmp(name, "tune_plane_stores") && value <= 1) sobel_nms_set_plane_store_variant(value); // process-wide
    else if (!std::strcmp(name, "gaussian_fma_div") && value <= 1) gaussian_set_fma_div(value != 0); // process-wide
    else if (!std::strcmp(name, "tune_finalize_mode") && value <= 1) hyst_set_finalize_mode(value);   // process-wide
    else if (!std::strcmp(name, "tune_gaussian_variant") && value <= 4) gaussian_set_march_variant(value); // process-wide
    else if (!std::strcmp(name, "tune_gaussian_seg") && value <= 8192) gaussian_set_seg_target(value);      // process-wide
    else return CANNY_HIP_ERR_INVALID;
    return CANNY_HIP_OK;
}

int canny_hip_synchronize(canny_hip_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc || (rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

const char *canny_hip_last_error(const canny_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }
int canny_hip_last_hysteresis_iterations(canny_hip_ctx *ctx)
{
    if (!ctx) return 0;
    if (ctx->hyst_iters_async && ctx->flags.p) {
        // the tail path never reports to the host: fetch the last sweep that scheduled work (diagnostic, synchronises)
        unsigned last = 0;
        if (hipSetDevice(ctx->device) == hipSuccess &&
            hipMemcpyAsync(&last, ctx->flags.p, sizeof last, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
            hipStreamSynchronize(ctx->stream) == hipSuccess)
            ctx->last_hyst_iters = (int)last + 1;
        else
            (void)hipGetLastError();
        ctx->hyst_iters_async = false;
    }
    return ctx->last_hyst_iters;
}

// ---- memory helpers -------------------------------------------------------------------------------
int canny_hip_malloc(canny_hip_ctx *ctx, void **dev_ptr, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!dev_ptr) return CANNY_HIP_ERR_INVALID;
    HIP_TRY(ctx, hipMalloc(dev_ptr, bytes ? bytes : 1));
    return CANNY_HIP_OK;
}
int canny_hip_free(canny_hip_ctx *ctx, void *dev_ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipFree(dev_ptr));
    return CANNY_HIP_OK;
}
// Pinned memory NEXT TO THE GPU: the pages of a hipHostMalloc come from the NUMA node of the CPU the calling thread
// happens to run on, and a buffer on the other socket costs the batch pipeline a third to a half of the PCIe rate
// (measured on a two-socket MI355X host: 11.5-19 instead of 25.4 Gpix/s, differing from run to run with the
// scheduler's choice).  So the allocation and the first touch of every page happen with the thread bound to the
// GPU's local CPUs (sysfs local_cpulist); the thread's own affinity is restored afterwards.
int canny_hip_host_alloc(canny_hip_ctx *ctx, void **host_ptr, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!host_ptr) return CANNY_HIP_ERR_INVALID;
    hipError_t e = numa_host_malloc(ctx->device, host_ptr, bytes);
    HIP_TRY(ctx, e);
    return CANNY_HIP_OK;
}
int canny_hip_host_free(canny_hip_ctx *ctx, void *host_ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipHostFree(host_ptr));
    return CANNY_HIP_OK;
}
// Page-locks memory the caller allocated itself (new[], malloc, a cv::Mat's data ...), so that the batch entry
// points DMA it in place like memory from canny_hip_host_alloc.  ~22 ms per GB the first time on an MI355X host.
int canny_hip_host_register(canny_hip_ctx *ctx, void *host_ptr, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!host_ptr || !bytes) return CANNY_HIP_ERR_INVALID;
    HIP_TRY(ctx, hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
    return CANNY_HIP_OK;
}
int canny_hip_host_unregister(canny_hip_ctx *ctx, void *host_ptr)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!host_ptr) return CANNY_HIP_ERR_INVALID;
    HIP_TRY(ctx, hipHostUnregister(host_ptr));
    return CANNY_HIP_OK;
}
int canny_hip_memcpy_h2d(canny_hip_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}
int canny_hip_memcpy_d2h(canny_hip_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes)
{
    int rc = bind(ctx);
    if (rc) return rc;
    return d2h_sync(ctx, host_dst, dev_src, bytes);
}

// ---- host-pointer stage functions -----------------------------------------------------------------
int canny_hip_gaussian_kernel(float sigma, float *taps, int cap, int *window)
{
    if (!taps || !window) return CANNY_HIP_ERR_INVALID;
    GaussTaps t;
    int rc = make_taps(sigma, t);
    if (rc) return rc;
    int w = 2 * t.center + 1;
    *window = w;
    if (cap < w) return CANNY_HIP_ERR_INVALID;
    std::memcpy(taps, t.tap, (size_t)w * sizeof(float));
    return CANNY_HIP_OK;
}

int canny_hip_gaussian(canny_hip_ctx *ctx, const unsigned char *img, float sigma, int height, int width, short *result)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!img || !result) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    size_t n = npx(height, width, 1);
    if ((rc = h2d(ctx, ctx->io[0], img, n))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(n * 2));
    if ((rc = dev_gaussian(ctx, (const unsigned char *)ctx->io[0].p, sigma, height, width, 1, (short *)ctx->io[1].p)))
        return rc;
    return d2h_sync(ctx, result, ctx->io[1].p, n * 2);
}

int canny_hip_xy_gradient(canny_hip_ctx *ctx, const short *img, int height, int width, short *grad_x, short *grad_y)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!img || !grad_x || !grad_y) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    if (height < 2 || width < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    size_t n = npx(height, width, 1);
    if ((rc = h2d(ctx, ctx->io[0], img, n * 2))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(n * 2));
    HIP_TRY(ctx, ctx->io[2].ensure(n * 2));
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_XY_GRADIENT);
        HIP_TRY(ctx, launch_xy_gradient((const int16_t *)ctx->io[0].p, (int16_t *)ctx->io[1].p, (int16_t *)ctx->io[2].p,
                                        height, width, 1, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(grad_x, ctx->io[1].p, n * 2, hipMemcpyDeviceToHost, ctx->stream));
    return d2h_sync(ctx, grad_y, ctx->io[2].p, n * 2);
}

int canny_hip_sobel(canny_hip_ctx *ctx, const short *img, int height, int width, short *magnitude, short *angle)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!img || !magnitude || !angle) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    if (height < 2 || width < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    size_t n = npx(height, width, 1);
    if ((rc = h2d(ctx, ctx->io[0], img, n * 2))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(n * 2));
    HIP_TRY(ctx, ctx->io[2].ensure(n * 2));
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL);
        HIP_TRY(ctx, launch_sobel((const int16_t *)ctx->io[0].p, (int16_t *)ctx->io[1].p, (int16_t *)ctx->io[2].p,
                                  height, width, 1, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(magnitude, ctx->io[1].p, n * 2, hipMemcpyDeviceToHost, ctx->stream));
    return d2h_sync(ctx, angle, ctx->io[2].p, n * 2);
}

int canny_hip_nms(canny_hip_ctx *ctx, const short *magnitude, const short *angle, int height, int width, short *result)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!magnitude || !angle || !result) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    size_t n = npx(height, width, 1);
    if ((rc = h2d(ctx, ctx->io[0], magnitude, n * 2))) return rc;
    if ((rc = h2d(ctx, ctx->io[1], angle, n * 2))) return rc;
    HIP_TRY(ctx, ctx->io[2].ensure(n * 2));
    {
        StageTimer tm(ctx, CANNY_HIP_STAGE_NMS);
        HIP_TRY(ctx, launch_nms((const int16_t *)ctx->io[0].p, (const int16_t *)ctx->io[1].p, (int16_t *)ctx->io[2].p,
                                height, width, 1, ctx->stream));
    }
    return d2h_sync(ctx, result, ctx->io[2].p, n * 2);
}

int canny_hip_hysteresis(canny_hip_ctx *ctx, short *edge_candidates, int height, int width, int min_val, int max_val)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!edge_candidates) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    size_t n = npx(height, width, 1);
    if ((rc = h2d(ctx, ctx->io[0], edge_candidates, n * 2))) return rc;
    if ((rc = dev_hysteresis(ctx, (short *)ctx->io[0].p, height, width, 1, min_val, max_val))) return rc;
    return d2h_sync(ctx, edge_candidates, ctx->io[0].p, n * 2);
}

int canny_hip_find_edge_pixels(canny_hip_ctx *ctx, short *edge_candidates, unsigned char *visited, int start,
                               int min_val, int max_val, int height, int width)
{
    (void)max_val; // unused by the reference too (src/utils.cpp:360-427)
    int rc = bind(ctx);
    if (rc) return rc;
    if (!edge_candidates || !visited) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    size_t n = npx(height, width, 1);
    if (start < 0 || (size_t)start >= n) return CANNY_HIP_ERR_INVALID;
    if (visited[start]) return CANNY_HIP_OK; // src/utils.cpp:361
    // min_val > EDGE: a popped pixel (now 255) fails the `>= minVal` test of its neighbours' checks, which changes
    // the reference's visited bookkeeping of the start pixel with the pop order
    if (min_val > 255) return CANNY_HIP_ERR_DOMAIN;
    HystGeom g = make_hyst_geom(height, width, 1);
    if ((rc = finish_pending(ctx))) return rc; // a streamed call's sweeps own the planes until they are done
    if ((rc = ensure_hyst(ctx, g))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], edge_candidates, n * 2))) return rc;
    if ((rc = h2d(ctx, ctx->io[1], visited, n))) return rc;
    if ((rc = prepare_hyst(ctx, g, /*zero_pad=*/false))) return rc;
    HIP_TRY(ctx, launch_fep_classify((const int16_t *)ctx->io[0].p, (const uint8_t *)ctx->io[1].p,
                                     (uint64_t *)ctx->plane_s.p, (uint64_t *)ctx->plane_c.p, g, start, min_val,
                                     ctx->stream));
    // fep_finalize updates its inputs in place, so it runs once, after convergence (not speculatively)
    rc = run_propagation(ctx, g, /*speculative=*/false, [&]() -> int {
        HIP_TRY(ctx, launch_fep_finalize((int16_t *)ctx->io[0].p, (uint8_t *)ctx->io[1].p,
                                         (const uint64_t *)ctx->plane_s.p, g, start, min_val, ctx->stream));
        return CANNY_HIP_OK;
    });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(edge_candidates, ctx->io[0].p, n * 2, hipMemcpyDeviceToHost, ctx->stream));
    return d2h_sync(ctx, visited, ctx->io[1].p, n);
}

enum MapFormat { kMapS16 = 0, kMapU8 = 1, kMapBits = 2 };
// Per-frame thresholds of a batch call, on HOST memory: explicit pairs (2 * n_frames ints, already validated), or an
// automatic rule whose selected pairs go to `out` (2 * n_frames ints, or null).
struct BatchThr {
    const int *pairs = nullptr;
    int rule = 0;
    double low = 0.0, high = 0.0;
    int *out = nullptr;
};
static int canny_batch_impl(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                            int max_val, int height, int width, void *edges, MapFormat fmt,
                            const ColorIn *color = nullptr, const BatchThr *bthr = nullptr);

int canny_hip_canny(canny_hip_ctx *ctx, const unsigned char *img, float sigma, int min_val, int max_val, int height,
                    int width, short *edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!img || !edges) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    size_t n = npx(height, width, 1);
    // Frames of a megapixel and more go through the batch pipeline as a batch of one: pinned staging for the upload and
    // the compact transfer for the map (1/16 of the bytes down, host threads write the caller's plane) -- the caller's
    // buffers here are ordinary new[] / cv::Mat memory, for which a plain 2-byte-per-pixel download is slowest of all.
    if (n >= (1u << 20) && height >= 2 && width >= 2 && ctx->batch_compact != 1)
        return canny_batch_impl(ctx, img, 1, sigma, min_val, max_val, height, width, edges, kMapS16);
    if ((rc = h2d(ctx, ctx->io[0], img, n))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(n * 2));
    if ((rc = dev_canny(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, 1,
                        (short *)ctx->io[1].p)))
        return rc;
    return d2h_sync(ctx, edges, ctx->io[1].p, n * 2);
}

int canny_hip_shard_range(int n_frames, int rank, int world, int *begin, int *end)
{
    if (!begin || !end || world < 1 || rank < 0 || rank >= world || n_frames < 0) return CANNY_HIP_ERR_INVALID;
    // contiguous ranges, the first (n_frames % world) shards one frame longer
    long long q = n_frames / world, r = n_frames % world;
    long long b = rank * q + std::min<long long>(rank, r);
    long long e = b + q + (rank < r ? 1 : 0);
    *begin = (int)b;
    *end = (int)e;
    return CANNY_HIP_OK;
}

// Stream-overlapped batch (BASELINE config 3).  The frames are cut into chunks; every pipeline (BatchPipe: one host
// thread, an upload, a compute and a download stream, three chunk slots) takes every n-th chunk and runs
//     upload(j+1) | kernels(j) | download(j-1)
// concurrently, chained by events only: the host thread never waits for a copy, it only blocks where
// canny() itself does (the hysteresis convergence poll at the end of a chunk's kernels), by which time the next
// chunk's upload has long been queued.  On an MI355X the kernels run at ~450 Gpix/s and a PCIe 5 x16 link moves
// ~56 GB/s per direction (48 + 48 GB/s with both directions busy): the link is the bound, and the pipeline's job is
// to keep both DMA engines busy all the time.
//   pinned caller buffers (canny_hip_host_alloc, hipHostMalloc, hipHostRegister): DMA'd in place, one pipeline;
//   pageable caller buffers: staged through the slot's pinned buffers by the pipeline's own thread (memcpy), so
//   several pipelines run side by side to get enough copy bandwidth.
// What a batch call returns per frame: the reference's short plane (0 / 255), the same as bytes, or one bit per pixel
// (rows MSB-first, padded to whole bytes -- launch_edges_to_bits).
static size_t map_frame_bytes(MapFormat fmt, int height, int width)
{
    if (fmt == kMapBits) return (size_t)height * (size_t)((width + 7) / 8);
    return npx(height, width, 1) * (fmt == kMapU8 ? 1 : sizeof(short));
}

// color: interleaved colour frames (CH bytes per pixel): chunks, staging and uploads are sized in input bytes
// bthr: per-frame thresholds (BatchThr); each chunk's pairs travel through the slot's small pinned buffer on the compute
// stream, so frame f keeps its pair whatever the chunking, the number of pipelines or the transfer mode
static int canny_batch_impl(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                            int max_val, int height, int width, void *edges, MapFormat fmt, const ColorIn *color,
                            const BatchThr *bthr)
{
    using Pipe = canny_hip_ctx::BatchPipe;
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !edges) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, 1))) return rc;
    if (n_frames < 1) return CANNY_HIP_ERR_INVALID;
    if (height < 2 || width < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    GaussTaps probe;
    if ((rc = make_taps(sigma, probe))) return rc;
    const size_t frame_px = npx(height, width, 1);
    const size_t frame_in = frame_px * (color ? (size_t)color->ch : 1u); // input bytes of one frame
    const int device = ctx->device;
    // Buffers from canny_hip_host_alloc (or any hipHostMalloc / hipHostRegister'd memory) need no staging.
    auto is_pinned = [](const void *p) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return attr.type == hipMemoryTypeHost;
    };
    // Compact transfer (s16 and u8 maps): the device packs the map into bits, the bits travel, host threads expand them
    // into the caller's plane (ExpandPool).  The caller's output buffer is then written by CPU stores: it needs no
    // pinning and no staging copy.
    const bool compact = fmt != kMapBits && ctx->batch_compact != 1;
    if (ctx->batch_compact != 1 && !ctx->expand_pool) { // (also stages pageable input frames, see below)
        // 8 threads (profiles/r03/compact_transfer_threads_chunks.txt, 128 x 4K: 2 / 4 / 8 / 16 / 24 threads 52.7 / 53.0 /
        // 53.1 / 52.7 / 52.4 Gpix/s, 12 threads 49.8 both times it was measured, the plain download 25.4): even two
        // keep up with one GPU's upload -- streaming stores, and the pipeline thread works on blocks while it waits --,
        // so this is headroom for slower hosts.  Never more than the CPUs this thread may run on (the sharder and
        // bench.py bind themselves to the GPU's local CPUs first, and the pool's threads inherit that mask)
        int n = ctx->batch_expand_threads;
        if (n <= 0) {
            cpu_set_t set;
            const int avail = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 1;
            n = std::max(1, std::min(8, avail - 1));
        }
        ctx->expand_pool.reset(new (std::nothrow) ExpandPool(n));
        if (!ctx->expand_pool) return CANNY_HIP_ERR_RUNTIME;
    }
    const bool in_pinned = is_pinned(imgs), out_pinned = compact ? false : is_pinned(edges);
    // Pageable INPUT frames are staged into the chunk slot's pinned buffer by the same pool (1 MB pieces, the
    // pipeline thread works too): ~90 GB/s of memcpy against the link's 54, so ordinary caller memory runs through
    // the same single three-stream pipeline as pinned memory.  (Rounds 1-2: six single-stream pipelines whose
    // threads each copied their own chunks -- 20-35 Gpix/s and bimodal from call to call.)
    const bool pool_staging = !in_pinned && ctx->expand_pool != nullptr;
    const bool all_pinned = (in_pinned || pool_staging) && (out_pinned || compact);
    // Defaults from the sweep on an MI355X box (tools/probe_batch_sweep.py, 128 x 4K and 256 x 1080p):
    //   pinned buffers:   ONE three-stream pipeline, 24 MB chunks -- s16 maps 25.3 Gpix/s (D2H 50.6 GB/s: the link's
    //                     rate with both directions busy), u8 maps 45.4 Gpix/s; a second pipeline only adds streams
    //                     that fight for hardware queues (20.9 / 33.2);
    //   pageable buffers: six single-stream pipelines, 8 MB chunks (the staging memcpys need the threads): 21.9 /
    //                     32.4 Gpix/s.
    // "tune_batch_pipe_mode": 1 = three streams, 2 = one in-order stream per pipeline, 0 = automatic.
    const bool three_streams = ctx->batch_pipe_mode ? ctx->batch_pipe_mode == 1 : all_pinned;
    size_t chunk_frames = ctx->batch_chunk_frames
                              ? (size_t)ctx->batch_chunk_frames
                              : ((size_t)(ctx->batch_chunk_mb ? ctx->batch_chunk_mb : (all_pinned ? 24 : 8)) << 20) / frame_in;
    // never more than the 65535 frames a launch takes
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)n_frames, 65535), chunk_frames));
    const int n_chunks = (n_frames + chunk - 1) / chunk;
    const int n_workers = std::min(ctx->batch_workers ? ctx->batch_workers : (all_pinned ? 1 : 6), n_chunks);
    std::vector<int> status(n_workers, CANNY_HIP_OK);
    std::vector<std::string> errors(n_workers);
    while ((int)ctx->batch_pool.size() < n_workers) { // (sub-contexts are created here, on the caller's thread)
        Pipe *w = nullptr;
        if ((rc = create_batch_pipe(ctx, ctx->batch_pool.empty(), &w))) return rc;
        ctx->batch_pool.push_back(w);
    }
    if (three_streams)
        for (int i = 0; i < n_workers; i++)
            if ((rc = ensure_copy_streams(ctx, *ctx->batch_pool[i]))) return rc;
    const size_t out_frame = map_frame_bytes(fmt, height, width); // bytes of one frame's map as the caller gets it
    const size_t bits_frame = map_frame_bytes(kMapBits, height, width);
    const size_t wire_frame = compact ? bits_frame : out_frame;   // ... and as it crosses the link
    const int row_bytes = (width + 7) / 8;

    auto worker = [&](int wid) {
        Pipe &P = *ctx->batch_pool[wid];
        canny_hip_ctx *sub = P.sub;
        int &st = status[wid];
        // single-stream mode: uploads and downloads in order on the compute stream (overlap only between pipelines)
        const hipStream_t s_h2d = three_streams ? P.s_h2d : sub->stream;
        const hipStream_t s_d2h = three_streams ? P.s_d2h : sub->stream;
        if (hipSetDevice(device) != hipSuccess) { // a new thread starts on device 0
            st = CANNY_HIP_ERR_RUNTIME;
            return;
        }
        const int my_chunks = (n_chunks - wid + n_workers - 1) / n_workers;
        const size_t in_bytes = frame_in * chunk, out_bytes = wire_frame * chunk;
        hipError_t e = hipSuccess;
        constexpr int n_slots = Pipe::kSlots;
        for (int k = 0; k < std::min(my_chunks, n_slots) && e == hipSuccess; k++) {
            Pipe::Slot &S = P.slot[k];
            S.d2h_issued = false;
            S.retire_dst = nullptr;
            S.expand_left.store(0);
            // pageable caller buffers are staged through pinned memory; pinned ones are DMA'd in place
            if (!in_pinned) e = S.pin_in.ensure(in_bytes, device);
            if (e == hipSuccess && !out_pinned) e = S.pin_out.ensure(out_bytes, device);
            if (e == hipSuccess) e = S.d_in.ensure(in_bytes);
            if (e == hipSuccess) e = S.d_out.ensure(frame_px * chunk * sizeof(short));
            if (e == hipSuccess && (fmt != kMapS16 || compact)) e = S.d_out8.ensure(out_bytes);
            if (e == hipSuccess && bthr) e = S.d_thr.ensure((size_t)chunk * 2 * sizeof(int));
            if (e == hipSuccess && bthr) e = S.pin_thr.ensure((size_t)chunk * 2 * sizeof(int), device);
        }
        if (e != hipSuccess) {
            st = fail(sub, e, "batch staging allocation");
            errors[wid] = sub->last_error;
            return;
        }
        auto chunk_range = [&](int j, int &f0, int &nf) {
            const int c = wid + j * n_workers;
            f0 = c * chunk;
            nf = std::min(chunk, n_frames - f0);
        };
        // host -> d_in of chunk j
        auto upload = [&](int j) -> hipError_t {
            Pipe::Slot &S = P.slot[j % n_slots];
            int f0, nf;
            chunk_range(j, f0, nf);
            const unsigned char *src = imgs + (size_t)f0 * frame_in;
            hipError_t err = hipSuccess;
            if (j >= n_slots) {
                // the slot's previous user (chunk j - kSlots): its kernels must have read d_in (dev_canny no longer
                // blocks the host), and its upload must have left pin_in
                err = hipStreamWaitEvent(s_h2d, S.ev_comp, 0);
                if (err == hipSuccess && !in_pinned) err = hipEventSynchronize(S.ev_h2d);
                if (err != hipSuccess) return err;
            }
            if (!in_pinned) {
                if (pool_staging)
                    ctx->expand_pool->parallel_copy(S.pin_in.p, src, frame_in * nf);
                else
                    std::memcpy(S.pin_in.p, src, frame_in * nf);
                src = (const unsigned char *)S.pin_in.p;
            }
            err = hipMemcpyAsync(S.d_in.p, src, frame_in * nf, hipMemcpyHostToDevice, s_h2d);
            if (err == hipSuccess) err = hipEventRecord(S.ev_h2d, s_h2d);
            return err;
        };
        // the staged output of chunk j reaches the caller's pageable buffer
        auto retire = [&](int j) -> hipError_t {
            Pipe::Slot &S = P.slot[j % n_slots];
            if (!S.retire_dst) return hipSuccess;
            hipError_t err = hipEventSynchronize(S.ev_d2h);
            if (err == hipSuccess && compact) {
                // the chunk's bit maps have landed in pin_out: hand them to the expansion pool in blocks of rows and
                // go on (the pool's threads write the caller's plane while the next chunks move)
                constexpr int kBlockRows = 128;
                const int blocks_per_frame = (height + kBlockRows - 1) / kBlockRows;
                S.expand_left.store(S.retire_frames * blocks_per_frame, std::memory_order_release);
                const size_t px_bytes = fmt == kMapU8 ? 1 : sizeof(short);
                for (int f = 0; f < S.retire_frames; f++)
                    for (int b = 0; b < blocks_per_frame; b++) {
                        const int r0 = b * kBlockRows;
                        ExpandPool::Job job;
                        job.bits = (const uint8_t *)S.pin_out.p + (size_t)f * bits_frame + (size_t)r0 * row_bytes;
                        job.dst = (unsigned char *)S.retire_dst + ((size_t)f * frame_px + (size_t)r0 * width) * px_bytes;
                        job.rows = std::min(kBlockRows, height - r0);
                        job.width = width;
                        job.row_bytes = row_bytes;
                        job.to_u8 = fmt == kMapU8;
                        job.left = &S.expand_left;
                        ctx->expand_pool->submit(job);
                    }
            } else if (err == hipSuccess) {
                std::memcpy(S.retire_dst, S.pin_out.p, S.retire_bytes);
            }
            S.retire_dst = nullptr;
            return err;
        };
        const char *where = "batch H2D";
        e = upload(0);
        for (int j = 0; j < my_chunks && e == hipSuccess && st == CANNY_HIP_OK; j++) {
            Pipe::Slot &S = P.slot[j % n_slots];
            int f0, nf;
            chunk_range(j, f0, nf);
            if (j + 1 < my_chunks && (e = upload(j + 1)) != hipSuccess) break;
            // kernels of chunk j: behind its upload, and behind the download that last read this slot's outputs
            where = "batch compute";
            if ((e = hipStreamWaitEvent(sub->stream, S.ev_h2d, 0)) != hipSuccess) break;
            if (S.d2h_issued && (e = hipStreamWaitEvent(sub->stream, S.ev_d2h, 0)) != hipSuccess) break;
            ThrSpec spec;
            const size_t thr_bytes = (size_t)nf * 2 * sizeof(int);
            if (bthr) {
                // pin_thr is free: the slot's previous chunk was waited for (ev_comp) before its download was queued
                spec.rule = bthr->rule;
                spec.low = bthr->low;
                spec.high = bthr->high;
                if (bthr->rule) {
                    spec.out = (int *)S.d_thr.p;
                } else {
                    std::memcpy(S.pin_thr.p, bthr->pairs + 2 * (size_t)f0, thr_bytes);
                    if ((e = hipMemcpyAsync(S.d_thr.p, S.pin_thr.p, thr_bytes, hipMemcpyHostToDevice, sub->stream)) !=
                        hipSuccess)
                        break;
                    spec.pairs = (const int *)S.d_thr.p;
                }
            }
            st = dev_canny(sub, (const unsigned char *)S.d_in.p, sigma, min_val, max_val, height, width, nf,
                           (short *)S.d_out.p, color, bthr ? &spec : nullptr);
            if (st) break;
            if (bthr && bthr->rule && bthr->out &&
                (e = hipMemcpyAsync(S.pin_thr.p, S.d_thr.p, thr_bytes, hipMemcpyDeviceToHost, sub->stream)) != hipSuccess)
                break;
            const void *d_res = S.d_out.p;
            if (fmt != kMapS16 || compact) { // narrow on the device: the D2H copy is what these variants are for
                e = (fmt == kMapU8 && !compact)
                        ? launch_edges_to_u8((const int16_t *)S.d_out.p, (uint8_t *)S.d_out8.p, frame_px * nf, sub->stream)
                        : launch_edges_to_bits((const int16_t *)S.d_out.p, (uint8_t *)S.d_out8.p, height, width, nf,
                                               sub->stream);
                if (e != hipSuccess) break;
                d_res = S.d_out8.p;
            }
            if ((e = hipEventRecord(S.ev_comp, sub->stream)) != hipSuccess) break;
            // The HOST waits for chunk j's kernels here (its next upload is already queued).  canny() itself no longer
            // blocks, and a host that runs ahead by the whole batch -- a thousand queued copies, kernels and event
            // waits -- makes the runtime slower per chunk and erratic: 1024 x 1080p in 24 MB chunks 18.7 Gpix/s
            // against 25.5 with a third as many 64 MB chunks, 128 x 4K anywhere between 19 and 25.4 from run to run.
            // One chunk of run-ahead is what the blocking canny() of the first version of this pipeline gave it,
            // and what measured best and steadiest (profiles/r02/c3_sweep_*.txt, pipe_patterns.txt "P2b"); letting
            // the host run five chunks ahead kept the s16 rate but made the u8 rate erratic (27-44 ms per 128 x 4K).
            if ((e = hipEventSynchronize(S.ev_comp)) != hipSuccess) break;
            if (bthr && bthr->rule && bthr->out) std::memcpy(bthr->out + 2 * (size_t)f0, S.pin_thr.p, thr_bytes);
            // download of chunk j (pin_out of this slot was retired kSlots - 1 iterations ago)
            where = "batch D2H";
            unsigned char *dst = (unsigned char *)edges + (size_t)f0 * out_frame;
            const size_t bytes = wire_frame * nf;
            // compact transfer: the expansion of the chunk that used this slot's pin_out before must have read it
            if (compact) ctx->expand_pool->wait(S.expand_left);
            if ((e = hipStreamWaitEvent(s_d2h, S.ev_comp, 0)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(out_pinned ? (void *)dst : S.pin_out.p, d_res, bytes, hipMemcpyDeviceToHost,
                                    s_d2h)) != hipSuccess)
                break;
            if ((e = hipEventRecord(S.ev_d2h, s_d2h)) != hipSuccess) break;
            S.d2h_issued = true;
            if (!out_pinned) {
                S.retire_dst = dst;
                S.retire_bytes = bytes;
                S.retire_frames = nf;
            }
            if (j > 0 && (e = retire(j - 1)) != hipSuccess) break;
        }
        if (e == hipSuccess && st == CANNY_HIP_OK && my_chunks > 0) e = retire(my_chunks - 1);
        if (compact) // every plane block of this pipeline has been written when the call returns (also after errors)
            for (auto &sl : P.slot) ctx->expand_pool->wait(sl.expand_left);
        // nothing of this call may still be in flight when it returns (also after an error: the slots are reused)
        hipError_t e2 = hipStreamSynchronize(s_h2d);
        hipError_t e3 = hipStreamSynchronize(sub->stream);
        hipError_t e4 = hipStreamSynchronize(s_d2h);
        if (e == hipSuccess) e = e2 != hipSuccess ? e2 : (e3 != hipSuccess ? e3 : e4);
        if (e != hipSuccess && st == CANNY_HIP_OK) st = fail(sub, e, where);
        if (st != CANNY_HIP_OK) errors[wid] = sub->last_error;
    };
    std::vector<std::thread> threads;
    for (int i = 1; i < n_workers; i++) threads.emplace_back(worker, i);
    worker(0);
    for (auto &t : threads) t.join();
    for (int i = 0; i < n_workers; i++)
        if (status[i]) {
            ctx->last_error = errors[i];
            return status[i];
        }
    return CANNY_HIP_OK;
}

int canny_hip_canny_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                          int max_val, int height, int width, short *edges)
{
    return canny_batch_impl(ctx, imgs, n_frames, sigma, min_val, max_val, height, width, edges, kMapS16);
}

int canny_hip_canny_batch_u8(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                             int max_val, int height, int width, unsigned char *edges)
{
    return canny_batch_impl(ctx, imgs, n_frames, sigma, min_val, max_val, height, width, edges, kMapU8);
}

int canny_hip_canny_batch_bits(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                               int max_val, int height, int width, unsigned char *bits)
{
    return canny_batch_impl(ctx, imgs, n_frames, sigma, min_val, max_val, height, width, bits, kMapBits);
}

// ---- per-frame thresholds ------------------------------------------------------
int canny_hip_auto_thresholds_from_histogram(const unsigned int *hist257, int rule, float low, float high, int *min_val,
                                             int *max_val)
{
    if (!hist257 || !min_val || !max_val || !auto_params_valid(rule, low, high)) return CANNY_HIP_ERR_INVALID;
    unsigned long long cum[kHistBins], run = 0;
    for (int b = 0; b < kHistBins; b++) cum[b] = run += hist257[b];
    if (run == 0) return CANNY_HIP_ERR_INVALID; // an empty histogram has no quantiles
    int lo, hi;
    auto_thresholds([&](int b) { return cum[b]; }, rule, (double)low, (double)high, lo, hi);
    *min_val = lo;
    *max_val = hi;
    return CANNY_HIP_OK;
}

int canny_hip_dev_canny_thresholds(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, const int *d_thresholds,
                                   int height, int width, int n_frames, short *d_edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_edges || !d_thresholds) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    ThrSpec spec;
    spec.pairs = d_thresholds;
    return dev_canny(ctx, d_img, sigma, 0, 0, height, width, n_frames, d_edges, nullptr, &spec);
}

int canny_hip_dev_canny_auto(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int rule, float low, float high,
                             int height, int width, int n_frames, short *d_edges, int *d_thresholds)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_edges || !auto_params_valid(rule, low, high)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    ThrSpec spec;
    spec.rule = rule;
    spec.low = low;
    spec.high = high;
    spec.out = d_thresholds;
    return dev_canny(ctx, d_img, sigma, 0, 0, height, width, n_frames, d_edges, nullptr, &spec);
}

int canny_hip_canny_batch_thresholds(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma,
                                     const int *thresholds, int height, int width, short *edges)
{
    if (!ctx || !thresholds || n_frames < 1) return CANNY_HIP_ERR_INVALID;
    for (int f = 0; f < n_frames; f++) { // host pairs must already lie in the domain: nothing is written otherwise
        const int lo = thresholds[2 * f], hi = thresholds[2 * f + 1];
        if (lo < 1 || lo > hi || hi > 255) return CANNY_HIP_ERR_INVALID;
    }
    BatchThr bt;
    bt.pairs = thresholds;
    return canny_batch_impl(ctx, imgs, n_frames, sigma, 0, 0, height, width, edges, kMapS16, nullptr, &bt);
}

int canny_hip_canny_batch_auto(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int rule,
                               float low, float high, int height, int width, short *edges, int *thresholds)
{
    if (!ctx || !auto_params_valid(rule, low, high)) return CANNY_HIP_ERR_INVALID;
    BatchThr bt;
    bt.rule = rule;
    bt.low = low;
    bt.high = high;
    bt.out = thresholds;
    return canny_batch_impl(ctx, imgs, n_frames, sigma, 0, 0, height, width, edges, kMapS16, nullptr, &bt);
}

// ---- colour input on host buffers --------------------------------------------------------------------
int canny_hip_to_gray(canny_hip_ctx *ctx, const unsigned char *src, int layout, int height, int width,
                      unsigned char *gray)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!src || !gray) return CANNY_HIP_ERR_INVALID;
    ColorIn ci;
    if ((rc = make_color_in(ctx, layout, ci)) || (rc = check_dims(height, width, 1))) return rc;
    const size_t n = npx(height, width, 1);
    if ((rc = h2d(ctx, ctx->io[0], src, n * ci.ch))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(n));
    if ((rc = dev_to_gray(ctx, (const unsigned char *)ctx->io[0].p, ci, height, width, 1, (unsigned char *)ctx->io[1].p)))
        return rc;
    return d2h_sync(ctx, gray, ctx->io[1].p, n);
}

int canny_hip_canny_color(canny_hip_ctx *ctx, const unsigned char *src, int layout, float sigma, int min_val,
                          int max_val, int height, int width, short *edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!src || !edges) return CANNY_HIP_ERR_INVALID;
    ColorIn ci;
    if ((rc = make_color_in(ctx, layout, ci)) || (rc = check_dims(height, width, 1))) return rc;
    const size_t n = npx(height, width, 1);
    // as canny_hip_canny: a megapixel and more goes through the batch pipeline as a batch of one
    if (n >= (1u << 20) && height >= 2 && width >= 2 && ctx->batch_compact != 1)
        return canny_batch_impl(ctx, src, 1, sigma, min_val, max_val, height, width, edges, kMapS16, &ci);
    if ((rc = h2d(ctx, ctx->io[0], src, n * ci.ch))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(n * 2));
    if ((rc = dev_canny(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, 1,
                        (short *)ctx->io[1].p, &ci)))
        return rc;
    return d2h_sync(ctx, edges, ctx->io[1].p, n * 2);
}

static int canny_batch_color_impl(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames, float sigma,
                                  int min_val, int max_val, int height, int width, void *edges, MapFormat fmt)
{
    if (!ctx) return CANNY_HIP_ERR_INVALID;
    ColorIn ci;
    int rc = make_color_in(ctx, layout, ci);
    if (rc) return rc;
    return canny_batch_impl(ctx, srcs, n_frames, sigma, min_val, max_val, height, width, edges, fmt, &ci);
}

int canny_hip_canny_batch_color(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames, float sigma,
                                int min_val, int max_val, int height, int width, short *edges)
{
    return canny_batch_color_impl(ctx, srcs, layout, n_frames, sigma, min_val, max_val, height, width, edges, kMapS16);
}

int canny_hip_canny_batch_color_u8(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames, float sigma,
                                   int min_val, int max_val, int height, int width, unsigned char *edges)
{
    return canny_batch_color_impl(ctx, srcs, layout, n_frames, sigma, min_val, max_val, height, width, edges, kMapU8);
}

int canny_hip_canny_batch_color_bits(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames,
                                     float sigma, int min_val, int max_val, int height, int width, unsigned char *bits)
{
    return canny_batch_color_impl(ctx, srcs, layout, n_frames, sigma, min_val, max_val, height, width, bits, kMapBits);
}

// ---- multi-GPU sharder (BASELINE config 5) -----------------------------------------------------------
// One context per shard, kept between calls (a context with its pipelines, streams and staging costs ~10-20 ms to
// build); one host thread per shard per call, bound to the CPUs that are local to the shard's GPU.
namespace {
struct MultiGpuState {
    std::mutex mu;
    std::vector<canny_hip_ctx *> shard_ctx; // index = shard
    std::vector<int> shard_dev;
    int batch_workers = 0, batch_chunk_mb = 0, batch_chunk_frames = 0, batch_pipe_mode = 0, batch_compact = 0;
    int allow_device_reuse = 0; // shards beyond the device count wrap around (testing the sharder on a small box)
    int numa_affinity = 1;
};
MultiGpuState g_mgpu;

} // namespace

static int multi_gpu_impl(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val, int height,
                          int width, void *edges, int n_devices, MapFormat fmt)
{
    if (!imgs || !edges || n_frames < 1 || height < 1 || width < 1) return CANNY_HIP_ERR_INVALID;
    int avail = 0;
    int rc = canny_hip_device_count(&avail);
    if (rc) return rc;
    if (avail < 1) return CANNY_HIP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lock(g_mgpu.mu); // one sharded call at a time per process
    if (n_devices <= 0) n_devices = avail;
    if (n_devices > avail && !g_mgpu.allow_device_reuse) n_devices = avail;
    if (n_devices > 64) return CANNY_HIP_ERR_INVALID;
    const int n_shards = n_devices;
    const size_t frame_px = npx(height, width, 1);
    const size_t out_frame = map_frame_bytes(fmt, height, width);
    // contexts are created here, on the caller's thread, and kept for the next call
    while ((int)g_mgpu.shard_ctx.size() < n_shards) {
        const int shard = (int)g_mgpu.shard_ctx.size();
        canny_hip_ctx *c = nullptr;
        if ((rc = canny_hip_ctx_create(&c, shard % avail))) return rc;
        g_mgpu.shard_ctx.push_back(c);
        g_mgpu.shard_dev.push_back(shard % avail);
    }
    std::vector<int> status(n_shards, CANNY_HIP_OK);
    auto worker = [&](int shard, bool own_thread) {
        int b = 0, e = 0;
        canny_hip_shard_range(n_frames, shard, n_shards, &b, &e);
        if (e <= b) return; // more shards than frames
        canny_hip_ctx *ctx = g_mgpu.shard_ctx[shard];
        ctx->batch_workers = g_mgpu.batch_workers;
        ctx->batch_chunk_mb = g_mgpu.batch_chunk_mb;
        ctx->batch_chunk_frames = g_mgpu.batch_chunk_frames;
        ctx->batch_pipe_mode = g_mgpu.batch_pipe_mode;
        ctx->batch_compact = g_mgpu.batch_compact;
        // run next to the GPU: this thread and the pipeline threads it starts inherit the mask.  The caller's own
        // thread (shard 0) gets its mask back afterwards.
        cpu_set_t local, saved;
        bool restore = false;
        if (g_mgpu.numa_affinity && device_local_cpus(g_mgpu.shard_dev[shard], &local)) {
            if (!own_thread) restore = sched_getaffinity(0, sizeof saved, &saved) == 0;
            if (own_thread || restore) (void)sched_setaffinity(0, sizeof local, &local); // best effort
        }
        status[shard] = canny_batch_impl(ctx, imgs + (size_t)b * frame_px, e - b, sigma, min_val, max_val, height,
                                         width, (unsigned char *)edges + (size_t)b * out_frame, fmt);
        if (restore) (void)sched_setaffinity(0, sizeof saved, &saved);
    };
    std::vector<std::thread> threads;
    for (int d = 1; d < n_shards; d++) threads.emplace_back(worker, d, true);
    worker(0, false);
    for (auto &t : threads) t.join();
    for (int s : status)
        if (s) return s;
    return CANNY_HIP_OK;
}

int canny_hip_canny_multi_gpu(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                              int height, int width, short *edges, int n_devices)
{
    return multi_gpu_impl(imgs, n_frames, sigma, min_val, max_val, height, width, edges, n_devices, kMapS16);
}

int canny_hip_canny_multi_gpu_u8(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                                 int height, int width, unsigned char *edges, int n_devices)
{
    return multi_gpu_impl(imgs, n_frames, sigma, min_val, max_val, height, width, edges, n_devices, kMapU8);
}

int canny_hip_canny_multi_gpu_bits(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                                   int height, int width, unsigned char *bits, int n_devices)
{
    return multi_gpu_impl(imgs, n_frames, sigma, min_val, max_val, height, width, bits, n_devices, kMapBits);
}

int canny_hip_multi_gpu_set_option(const char *name, int value)
{
    if (!name || value < 0) return CANNY_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lock(g_mgpu.mu);
    if (!std::strcmp(name, "tune_batch_workers") && value <= 16) g_mgpu.batch_workers = value;
    else if (!std::strcmp(name, "tune_batch_chunk_mb") && value <= 1024) g_mgpu.batch_chunk_mb = value;
    else if (!std::strcmp(name, "tune_batch_chunk_frames") && value <= 65535) g_mgpu.batch_chunk_frames = value;
    else if (!std::strcmp(name, "tune_batch_pipe_mode") && value <= 2) g_mgpu.batch_pipe_mode = value;
    else if (!std::strcmp(name, "tune_batch_compact") && value <= 1) g_mgpu.batch_compact = value;
    else if (!std::strcmp(name, "allow_device_reuse") && value <= 1) g_mgpu.allow_device_reuse = value;
    else if (!std::strcmp(name, "numa_affinity") && value <= 1) g_mgpu.numa_affinity = value;
    else return CANNY_HIP_ERR_INVALID;
    return CANNY_HIP_OK;
}

int canny_hip_multi_gpu_release(void)
{
    std::lock_guard<std::mutex> lock(g_mgpu.mu);
    for (canny_hip_ctx *c : g_mgpu.shard_ctx) canny_hip_ctx_destroy(c);
    g_mgpu.shard_ctx.clear();
    g_mgpu.shard_dev.clear();
    return CANNY_HIP_OK;
}

// Number of CPUs in a sysfs-style list ("0-3,8,10-11" -> 7), 0 if malformed: the parser behind the NUMA binding.
int canny_hip_selftest_cpulist_count(const char *text)
{
    if (!text) return 0;
    cpu_set_t set;
    return parse_cpulist(text, &set);
}

// CPUs local to `device` as sysfs lists them ("0-31,128-159"); what canny_hip_canny_multi_gpu binds a shard's
// threads to.  CANNY_HIP_ERR_UNSUPPORTED when the platform does not say.
int canny_hip_device_local_cpus(int device, char *buf, int cap)
{
    if (!buf || cap < 2) return CANNY_HIP_ERR_INVALID;
    int n = 0;
    int rc = canny_hip_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return CANNY_HIP_ERR_INVALID;
    cpu_set_t set;
    if (!device_local_cpus(device, &set)) return CANNY_HIP_ERR_UNSUPPORTED;
    std::string out;
    for (int c = 0; c < CPU_SETSIZE;) {
        if (!CPU_ISSET(c, &set)) {
            c++;
            continue;
        }
        int e = c;
        while (e + 1 < CPU_SETSIZE && CPU_ISSET(e + 1, &set)) e++;
        if (!out.empty()) out += ",";
        out += std::to_string(c);
        if (e > c) out += "-" + std::to_string(e);
        c = e + 1;
    }
    if ((int)out.size() + 1 > cap) return CANNY_HIP_ERR_INVALID;
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return CANNY_HIP_OK;
}

// ---- device-pointer stage functions ---------------------------------------------------------------
int canny_hip_dev_gaussian(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int height, int width,
                           int n_frames, short *d_result)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_result) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    return dev_gaussian(ctx, d_img, sigma, height, width, n_frames, d_result);
}

int canny_hip_dev_xy_gradient(canny_hip_ctx *ctx, const short *d_img, int height, int width, int n_frames,
                              short *d_grad_x, short *d_grad_y)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_grad_x || !d_grad_y) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    if (height < 2 || width < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    StageTimer tm(ctx, CANNY_HIP_STAGE_XY_GRADIENT);
    HIP_TRY(ctx, launch_xy_gradient(d_img, d_grad_x, d_grad_y, height, width, n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_dev_sobel(canny_hip_ctx *ctx, const short *d_img, int height, int width, int n_frames, short *d_magnitude,
                        short *d_angle)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_magnitude || !d_angle) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    if (height < 2 || width < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL);
    HIP_TRY(ctx, launch_sobel(d_img, d_magnitude, d_angle, height, width, n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_dev_nms(canny_hip_ctx *ctx, const short *d_magnitude, const short *d_angle, int height, int width,
                      int n_frames, short *d_result)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_magnitude || !d_angle || !d_result) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    StageTimer tm(ctx, CANNY_HIP_STAGE_NMS);
    HIP_TRY(ctx, launch_nms(d_magnitude, d_angle, d_result, height, width, n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_dev_sobel_nms(canny_hip_ctx *ctx, const short *d_smoothed, int height, int width, int n_frames,
                            short *d_nms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_smoothed || !d_nms) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    if (height < 2 || width < 2) return CANNY_HIP_ERR_UNSUPPORTED;
    return dev_sobel_nms(ctx, d_smoothed, height, width, n_frames, d_nms);
}

int canny_hip_dev_gaussian_u8(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int height, int width,
                              int n_frames, unsigned char *d_result)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_result) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    return dev_gaussian(ctx, d_img, sigma, height, width, n_frames, d_result, 1);
}

int canny_hip_dev_sobel_nms_u8in(canny_hip_ctx *ctx, const unsigned char *d_smoothed, int height, int width,
                                 int n_frames, short *d_nms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_smoothed || !d_nms) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    if (height < 2 || width < 2 || !sobel_nms_u8_input_supported()) return CANNY_HIP_ERR_UNSUPPORTED;
    StageTimer tm(ctx, CANNY_HIP_STAGE_SOBEL_NMS, nullptr, /*attached=*/true);
    HIP_TRY(ctx, launch_sobel_nms_march_u8in(d_smoothed, d_nms, height, width, n_frames, ctx->stream,
                                             ctx->tune_sobel_seg, tm.launch_events()));
    return CANNY_HIP_OK;
}

int canny_hip_dev_hysteresis(canny_hip_ctx *ctx, short *d_edge_candidates, int height, int width, int n_frames,
                             int min_val, int max_val)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_edge_candidates) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    return dev_hysteresis(ctx, d_edge_candidates, height, width, n_frames, min_val, max_val);
}

int canny_hip_dev_canny(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                        int height, int width, int n_frames, short *d_edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_edges) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    return dev_canny(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges);
}

int canny_hip_dev_to_gray(canny_hip_ctx *ctx, const unsigned char *d_src, int layout, int height, int width,
                          int n_frames, unsigned char *d_gray)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_src || !d_gray) return CANNY_HIP_ERR_INVALID;
    ColorIn ci;
    if ((rc = make_color_in(ctx, layout, ci)) || (rc = check_dims(height, width, n_frames))) return rc;
    return dev_to_gray(ctx, d_src, ci, height, width, n_frames, d_gray);
}

int canny_hip_dev_gaussian_u8_color(canny_hip_ctx *ctx, const unsigned char *d_src, int layout, float sigma, int height,
                                    int width, int n_frames, unsigned char *d_result)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_src || !d_result) return CANNY_HIP_ERR_INVALID;
    ColorIn ci;
    if ((rc = make_color_in(ctx, layout, ci)) || (rc = check_dims(height, width, n_frames))) return rc;
    if (ci.ch == 1) return dev_gaussian(ctx, d_src, sigma, height, width, n_frames, d_result, 1);
    return dev_gaussian_u8_color(ctx, d_src, ci, sigma, height, width, n_frames, d_result);
}

int canny_hip_dev_canny_color(canny_hip_ctx *ctx, const unsigned char *d_src, int layout, float sigma, int min_val,
                              int max_val, int height, int width, int n_frames, short *d_edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_src || !d_edges) return CANNY_HIP_ERR_INVALID;
    ColorIn ci;
    if ((rc = make_color_in(ctx, layout, ci)) || (rc = check_dims(height, width, n_frames))) return rc;
    return dev_canny(ctx, d_src, sigma, min_val, max_val, height, width, n_frames, d_edges, &ci);
}

int canny_hip_dev_canny_stream(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_edges) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    return dev_canny_stream(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges);
}

int canny_hip_dev_canny_stream_flush(canny_hip_ctx *ctx)
{
    int rc = bind(ctx);
    return rc ? rc : finish_pending(ctx);
}

int canny_hip_dev_canny_u8(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                           int height, int width, int n_frames, unsigned char *d_edges)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_edges) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames);
    HIP_TRY(ctx, ctx->edges16.ensure(n * sizeof(short)));
    if ((rc = dev_canny(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, (short *)ctx->edges16.p)))
        return rc;
    HIP_TRY(ctx, launch_edges_to_u8((const int16_t *)ctx->edges16.p, d_edges, n, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_dev_canny_bits(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                             int height, int width, int n_frames, unsigned char *d_bits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_bits) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames);
    HIP_TRY(ctx, ctx->edges16.ensure(n * sizeof(short)));
    if ((rc = dev_canny(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, (short *)ctx->edges16.p)))
        return rc;
    HIP_TRY(ctx, launch_edges_to_bits((const int16_t *)ctx->edges16.p, d_bits, height, width, n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

// ---- edge point lists ---------------------------------------------------------------------------------
int canny_hip_dev_canny_points(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, unsigned int *d_points,
                               unsigned long long capacity, unsigned long long *d_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_offsets || (!d_points && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const uint64_t *strong = nullptr;
    if ((rc = dev_canny_points_count(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, d_offsets,
                                     &strong)))
        return rc;
    if (!strong) return CANNY_HIP_OK;
    return dev_points_scatter(ctx, strong, nullptr, make_hyst_geom(height, width, n_frames), d_offsets, d_points,
                              capacity);
}

int canny_hip_dev_points_from_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                   unsigned int *d_points, unsigned long long capacity, unsigned long long *d_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_offsets || (!d_points && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames)) || (rc = finish_pending(ctx))) return rc;
    const HystGeom g = make_hyst_geom(height, width, n_frames);
    if ((rc = dev_points_count(ctx, nullptr, d_bits, g, d_offsets))) return rc;
    return dev_points_scatter(ctx, nullptr, d_bits, g, d_offsets, d_points, capacity);
}

int canny_hip_canny_points(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, unsigned int *points, unsigned long long capacity,
                           unsigned long long *offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !offsets || (!points && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(off_bytes));
    unsigned long long *d_offsets = (unsigned long long *)ctx->io[1].p;
    const uint64_t *strong = nullptr;
    if ((rc = dev_canny_points_count(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                     n_frames, nullptr, d_offsets, &strong)))
        return rc;
    // the offsets come down first: they say how many points there are to scatter and to download
    std::vector<unsigned long long> off((size_t)n_frames + 1);
    if ((rc = d2h_sync(ctx, off.data(), d_offsets, off_bytes))) return rc;
    const unsigned long long n_pts = std::min(off[n_frames], capacity);
    if (n_pts) {
        HIP_TRY(ctx, ctx->io[2].ensure((size_t)n_pts * sizeof(unsigned)));
        if ((rc = dev_points_scatter(ctx, strong, nullptr, make_hyst_geom(height, width, n_frames), d_offsets,
                                     (unsigned *)ctx->io[2].p, n_pts)) ||
            (rc = d2h_sync(ctx, points, ctx->io[2].p, (size_t)n_pts * sizeof(unsigned))))
            return rc;
    }
    std::memcpy(offsets, off.data(), off_bytes);
    return CANNY_HIP_OK;
}

int canny_hip_points_from_bits(const unsigned char *bits, int height, int width, unsigned int *points,
                               unsigned long long capacity, unsigned long long *count)
{
    if (!bits || !count || (!points && capacity)) return CANNY_HIP_ERR_INVALID;
    int rc = check_dims(height, width, 1);
    if (rc) return rc;
    const size_t row_bytes = ((size_t)width + 7) / 8;
    unsigned long long n = 0;
    for (int y = 0; y < height; y++) {
        const unsigned char *row = bits + (size_t)y * row_bytes;
        for (size_t xb = 0; xb < row_bytes; xb++) {
            unsigned v = row[xb];
            const int left = width - (int)(xb * 8); // pixels of this row from this byte on
            if (left < 8) v &= 0xffu << (8 - left); // the row's padding bits are not pixels
            while (v) {
                const int k = __builtin_clz(v) - 24; // MSB-first: the highest set bit is the leftmost pixel
                if (n < capacity) points[n] = (unsigned)((size_t)y * width + xb * 8 + k);
                n++;
                v &= ~(0x80u >> k);
            }
        }
    }
    *count = n;
    return CANNY_HIP_OK;
}

// ---- sub-pixel edgels (canny_edgels.hip) -----------------------------------------
namespace {

// dev_canny (unchanged), count + scan of its map as the point lists do it, timed as the edgels' layout part.  *strong_out
// as dev_canny_points_count.
int dev_canny_edgels_count(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int lo, int hi, int h, int w, int n,
                           short *d_edges, unsigned long long *d_offsets, const uint64_t **strong_out)
{
    int rc = dev_canny_map(ctx, d_img, sigma, lo, hi, h, w, n, d_edges, strong_out);
    if (rc) return rc;
    if (!*strong_out) {
        HIP_TRY(ctx, hipMemsetAsync(d_offsets, 0, ((size_t)n + 1) * sizeof(unsigned long long), ctx->stream));
        return CANNY_HIP_OK;
    }
    const HystGeom g = make_hyst_geom(h, w, n);
    HIP_TRY(ctx, ctx->points.ensure(g.n_frames * sizeof(unsigned long long) + (size_t)n * h * sizeof(uint32_t)));
    unsigned long long *totals = (unsigned long long *)ctx->points.p;
    uint32_t *row_words = (uint32_t *)(totals + g.n_frames);
    StageTimer tm(ctx, canny_hip_ctx::kProfEdgels + CANNY_HIP_EDGEL_PART_LAYOUT);
    HIP_TRY(ctx, launch_points_count(*strong_out, nullptr, g, row_words, ctx->stream));
    HIP_TRY(ctx, launch_points_scan(row_words, totals, d_offsets, g.height, g.n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

// the records, behind dev_canny_edgels_count on the same stream: the strong plane and the smoothed plane that call left
int dev_edgels_rows(canny_hip_ctx *ctx, const uint64_t *strong, const HystGeom &g, const unsigned long long *d_offsets,
                    int *d_edgels, unsigned *d_points, unsigned long long capacity)
{
    if (!capacity) return CANNY_HIP_OK;
    const uint32_t *row_words = (const uint32_t *)((const unsigned long long *)ctx->points.p + g.n_frames);
    StageTimer tm(ctx, canny_hip_ctx::kProfEdgels + CANNY_HIP_EDGEL_PART_REFINE);
    HIP_TRY(ctx, launch_edgels_rows(strong, g, ctx->smoothed.p, ctx->last_canny_u8 != 0, row_words, d_offsets, d_edgels,
                                    d_points, capacity, ctx->stream));
    return CANNY_HIP_OK;
}

} // namespace

int canny_hip_dev_canny_edgels(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, int *d_edgels,
                               unsigned long long capacity, unsigned long long *d_offsets, unsigned int *d_points)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_offsets || (!d_edgels && capacity) || ((uintptr_t)d_edgels & 15)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const uint64_t *strong = nullptr;
    if ((rc = dev_canny_edgels_count(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, d_offsets,
                                     &strong)))
        return rc;
    if (!strong) return CANNY_HIP_OK;
    return dev_edgels_rows(ctx, strong, make_hyst_geom(height, width, n_frames), d_offsets, d_edgels, d_points, capacity);
}

int canny_hip_dev_edgels_at(canny_hip_ctx *ctx, const void *d_plane, int plane_is_u8, int height, int width, int n_frames,
                            const unsigned int *d_points, const unsigned long long *d_point_offsets, int *d_edgels,
                            unsigned long long capacity)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_point_offsets || ((!d_edgels || !d_points) && capacity) || ((uintptr_t)d_edgels & 15) || height < 2 || width < 2)
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, height, width) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        d_plane = ctx->smoothed.p;
        plane_is_u8 = ctx->last_canny_u8;
    }
    if ((rc = finish_pending(ctx))) return rc;
    if (!capacity) return CANNY_HIP_OK;
    StageTimer tm(ctx, canny_hip_ctx::kProfEdgels + CANNY_HIP_EDGEL_PART_REFINE);
    HIP_TRY(ctx, launch_edgels_at(d_plane, plane_is_u8 != 0, height, width, n_frames, d_points, d_point_offsets, d_edgels,
                                  capacity, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_canny_edgels(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int *edgels, unsigned long long capacity,
                           unsigned long long *offsets, unsigned int *points)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !offsets || (!edgels && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(off_bytes));
    unsigned long long *d_offsets = (unsigned long long *)ctx->io[1].p;
    const uint64_t *strong = nullptr;
    if ((rc = dev_canny_edgels_count(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                     n_frames, nullptr, d_offsets, &strong)))
        return rc;
    // the offsets come down first: they say how many records there are to compute and to download
    std::vector<unsigned long long> off((size_t)n_frames + 1);
    if ((rc = d2h_sync(ctx, off.data(), d_offsets, off_bytes))) return rc;
    const unsigned long long n_rec = std::min(off[n_frames], capacity);
    if (n_rec) {
        const size_t rec_bytes = (size_t)n_rec * CANNY_HIP_EDGEL_INTS * sizeof(int);
        HIP_TRY(ctx, ctx->io[2].ensure(rec_bytes));
        if (points) HIP_TRY(ctx, ctx->io[3].ensure((size_t)n_rec * sizeof(unsigned)));
        if ((rc = dev_edgels_rows(ctx, strong, make_hyst_geom(height, width, n_frames), d_offsets, (int *)ctx->io[2].p,
                                  points ? (unsigned *)ctx->io[3].p : nullptr, n_rec)))
            return rc;
        if (points)
            HIP_TRY(ctx, hipMemcpyAsync(points, ctx->io[3].p, (size_t)n_rec * sizeof(unsigned), hipMemcpyDeviceToHost,
                                        ctx->stream));
        if ((rc = d2h_sync(ctx, edgels, ctx->io[2].p, rec_bytes))) return rc;
    }
    std::memcpy(offsets, off.data(), off_bytes);
    return CANNY_HIP_OK;
}

int canny_hip_dev_edgels_arith(canny_hip_ctx *ctx, const short *d_gx, const short *d_gy, size_t n_pairs,
                               unsigned int *d_mag, int *d_dir, const unsigned int *d_abc, size_t n_triples, int *d_t,
                               int *d_refined)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((n_pairs && (!d_gx || !d_gy || !d_mag || !d_dir)) || (n_triples && (!d_abc || !d_t || !d_refined)) ||
        (!n_pairs && !n_triples))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, launch_edgels_arith(d_gx, d_gy, n_pairs, d_mag, d_dir, d_abc, n_triples, d_t, d_refined, ctx->stream));
    return CANNY_HIP_OK;
}

static int profile_collect(canny_hip_ctx *ctx);

// What every canny_hip_<feature>_profile_get does: part `part` of the `parts` slots from `base` on.
static int profile_part_get(canny_hip_ctx *ctx, int base, int parts, int part, double *total_ms, long *launches)
{
    if (part < 0 || part >= parts || !total_ms || !launches) return CANNY_HIP_ERR_INVALID;
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = profile_collect(ctx))) return rc;
    *total_ms = ctx->total_ms[base + part];
    *launches = ctx->launches[base + part];
    return CANNY_HIP_OK;
}

int canny_hip_edgels_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfEdgels, CANNY_HIP_EDGEL_PARTS, part, total_ms, launches);
}

// Host-only: the launch plan of the index-driven edgel kernel (plan_edgels_at), outputs as canny_hip_selftest_launch_plan.
int canny_hip_selftest_edgels_plan(int n_frames, int height, int width, unsigned long long n_points,
                                   unsigned long long *out)
{
    if (!out || !n_points || height < 2 || width < 2 || check_dims(height, width, n_frames)) return CANNY_HIP_ERR_INVALID;
    const LaunchPlan p = plan_edgels_at(height, width, n_points);
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// ---- connected components ----------------------------------------------------------------------------
int canny_hip_dev_canny_components(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                   int height, int width, int n_frames, short *d_edges, int min_area, int *d_labels,
                                   unsigned char *d_kept_u8, int *d_stats, unsigned long long capacity,
                                   unsigned long long *d_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_offsets || (!d_stats && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    return dev_canny_components(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, min_area,
                                CcOut{d_labels, d_kept_u8, d_stats, capacity, d_offsets});
}

int canny_hip_dev_components_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                  int min_area, int *d_labels, unsigned char *d_kept_u8, int *d_stats,
                                  unsigned long long capacity, unsigned long long *d_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_offsets || (!d_stats && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames)) || (rc = finish_pending(ctx))) return rc;
    return dev_components(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), min_area,
                          CcOut{d_labels, d_kept_u8, d_stats, capacity, d_offsets});
}

int canny_hip_canny_components(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                               int max_val, int height, int width, int min_area, int *labels, unsigned char *kept_u8,
                               int *stats, unsigned long long capacity, unsigned long long *offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !offsets || (!stats && capacity)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames);
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    // the records of a frame cannot outnumber its pixels: a larger capacity buys nothing
    const unsigned long long cap = std::min<unsigned long long>(capacity, n);
    const size_t stats_bytes = (size_t)cap * CANNY_HIP_CC_STATS * sizeof(int);
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: offsets | stats | kept; the label plane has a block of its own
    const size_t stats_at = (off_bytes + 15) & ~(size_t)15, kept_at = (stats_at + stats_bytes + 15) & ~(size_t)15;
    HIP_TRY(ctx, ctx->io[1].ensure(kept_at + (kept_u8 ? n : 0)));
    if (labels) HIP_TRY(ctx, ctx->io[2].ensure(n * sizeof(int)));
    char *d = (char *)ctx->io[1].p;
    const CcOut out{labels ? (int *)ctx->io[2].p : nullptr, kept_u8 ? (unsigned char *)(d + kept_at) : nullptr,
                    cap ? (int *)(d + stats_at) : nullptr, cap, (unsigned long long *)d};
    if ((rc = dev_canny_components(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                   n_frames, nullptr, min_area, out)))
        return rc;
    // the offsets come down first: they say how many records there are to download
    std::vector<unsigned long long> off((size_t)n_frames + 1);
    if ((rc = d2h_sync(ctx, off.data(), out.offsets, off_bytes))) return rc;
    const unsigned long long n_rec = std::min(off[n_frames], cap);
    if (n_rec)
        HIP_TRY(ctx, hipMemcpyAsync(stats, out.stats, (size_t)n_rec * CANNY_HIP_CC_STATS * sizeof(int),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (labels) HIP_TRY(ctx, hipMemcpyAsync(labels, out.labels, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (kept_u8) HIP_TRY(ctx, hipMemcpyAsync(kept_u8, out.kept, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(offsets, off.data(), off_bytes);
    return CANNY_HIP_OK;
}

// The rule on one host bit map: two passes with a union-find over provisional labels.  Provisional labels are handed out
// in raster order and the smaller root always wins, so a component's root label is the one its first pixel received and
// ascending root labels are ascending first pixels.
int canny_hip_components_from_bits(const unsigned char *bits, int height, int width, int min_area, int *labels,
                                   int *stats, unsigned long long capacity, unsigned long long *count)
{
    if (!bits || !count || (!stats && capacity)) return CANNY_HIP_ERR_INVALID;
    int rc = check_dims(height, width, 1);
    if (rc) return rc;
    const size_t row_bytes = ((size_t)width + 7) / 8, n = (size_t)height * width;
    std::vector<int> own;
    if (!labels) {
        own.resize(n);
        labels = own.data();
    }
    std::vector<int> parent(1, 0); // provisional label -> a smaller label of the same component (itself: a root)
    auto find = [&](int x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    auto unite = [&](int a, int b) {
        a = find(a), b = find(b);
        if (a < b) parent[b] = a;
        else parent[a] = b;
        return a < b ? a : b;
    };
    auto set_at = [&](int y, int x) { return (bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7))) & 1; };
    for (int y = 0; y < height; y++) {
        int *row = labels + (size_t)y * width;
        const int *up = y ? row - width : nullptr;
        for (int x = 0; x < width; x++) {
            if (!set_at(y, x)) {
                row[x] = 0;
                continue;
            }
            int l = x ? row[x - 1] : 0;
            if (up)
                for (int dx = -1; dx <= 1; dx++) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= width || !up[xx]) continue;
                    l = l ? unite(l, up[xx]) : up[xx];
                }
            if (!l) {
                l = (int)parent.size();
                parent.push_back(l);
            }
            row[x] = l;
        }
    }
    const size_t n_prov = parent.size();
    // per root: area, box, first pixel
    std::vector<int> area(n_prov, 0), left(n_prov, INT_MAX), top(n_prov, INT_MAX), right(n_prov, -1), bottom(n_prov, -1),
        first(n_prov, -1);
    for (int y = 0; y < height; y++) {
        const int *row = labels + (size_t)y * width;
        for (int x = 0; x < width; x++) {
            if (!row[x]) continue;
            const int r = find(row[x]);
            if (!area[r]++) first[r] = (int)((size_t)y * width + x), top[r] = y;
            left[r] = std::min(left[r], x), right[r] = std::max(right[r], x), bottom[r] = y;
        }
    }
    std::vector<int> number(n_prov, 0);
    unsigned long long k = 0;
    for (size_t r = 1; r < n_prov; r++) {
        if (parent[r] != (int)r || area[r] < min_area) continue;
        if (k < capacity) {
            int *rec = stats + k * CANNY_HIP_CC_STATS;
            rec[CANNY_HIP_CC_STAT_LEFT] = left[r], rec[CANNY_HIP_CC_STAT_TOP] = top[r];
            rec[CANNY_HIP_CC_STAT_WIDTH] = right[r] - left[r] + 1, rec[CANNY_HIP_CC_STAT_HEIGHT] = bottom[r] - top[r] + 1;
            rec[CANNY_HIP_CC_STAT_AREA] = area[r], rec[CANNY_HIP_CC_STAT_FIRST] = first[r];
        }
        number[r] = (int)++k;
    }
    if (own.empty())
        for (size_t i = 0; i < n; i++)
            if (labels[i]) labels[i] = number[find(labels[i])];
    *count = k;
    return CANNY_HIP_OK;
}

// ---- outer contour chains ----------------------------------------------------------------------------
int canny_hip_dev_canny_contours(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                 int height, int width, int n_frames, short *d_edges, int min_area, int *d_stats,
                                 unsigned long long capacity, unsigned long long *d_offsets,
                                 unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                 unsigned long long *d_point_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CtOut out{d_stats, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    if (!d_img || !contour_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames))) return rc;
    return dev_canny_contours(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, min_area, out);
}

int canny_hip_dev_contours_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                int min_area, int *d_stats, unsigned long long capacity, unsigned long long *d_offsets,
                                unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                unsigned long long *d_point_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CtOut out{d_stats, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    if (!d_bits || !contour_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = finish_pending(ctx))) return rc;
    return dev_contours(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), min_area, out);
}

int canny_hip_canny_contours(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                             int max_val, int height, int width, int min_area, int *stats, unsigned long long capacity,
                             unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                             unsigned long long point_capacity, unsigned long long *point_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !contour_args_ok(CtOut{stats, capacity, offsets, chain_offsets, points, point_capacity, point_offsets}))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames);
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    // a frame has no more records than pixels and no more chain points than 8 per pixel and one per record
    const unsigned long long cap = std::min<unsigned long long>(capacity, n);
    const unsigned long long pcap = std::min<unsigned long long>(point_capacity, 9ull * n);
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: offsets | point_offsets | chain_offsets | stats | points
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t poff_at = up16(off_bytes), chain_at = up16(poff_at + off_bytes);
    const size_t stats_at = up16(chain_at + ((size_t)cap + 1) * sizeof(unsigned long long));
    const size_t points_at = up16(stats_at + (stats ? (size_t)cap * CANNY_HIP_CC_STATS * sizeof(int) : 0));
    HIP_TRY(ctx, ctx->io[1].ensure(points_at + (size_t)pcap * sizeof(int)));
    char *d = (char *)ctx->io[1].p;
    const CtOut out{stats && cap ? (int *)(d + stats_at) : nullptr,
                    cap,
                    (unsigned long long *)d,
                    (unsigned long long *)(d + chain_at),
                    pcap ? (int *)(d + points_at) : nullptr,
                    pcap,
                    (unsigned long long *)(d + poff_at)};
    if ((rc = dev_canny_contours(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                 n_frames, nullptr, min_area, out)))
        return rc;
    // the offsets come down first: they say how many records and points there are to download
    std::vector<unsigned long long> off(2 * ((size_t)n_frames + 1));
    HIP_TRY(ctx, hipMemcpyAsync(off.data(), out.offsets, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = d2h_sync(ctx, off.data() + n_frames + 1, out.point_offsets, off_bytes))) return rc;
    const unsigned long long n_rec = std::min(off[n_frames], cap);
    if (chain_offsets)
        HIP_TRY(ctx, hipMemcpyAsync(chain_offsets, out.chain_offsets, ((size_t)n_rec + 1) * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec && out.stats)
        HIP_TRY(ctx, hipMemcpyAsync(stats, out.stats, (size_t)n_rec * CANNY_HIP_CC_STATS * sizeof(int),
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_rec && pcap) {
        // chain_offsets is needed on the host to know where the records that fit end
        unsigned long long end = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&end, out.chain_offsets + n_rec, sizeof end, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const unsigned long long n_pts = std::min(end, pcap);
        if (n_pts) {
            HIP_TRY(ctx, hipMemcpyAsync(points, out.points, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    std::memcpy(offsets, off.data(), off_bytes);
    std::memcpy(point_offsets, off.data() + n_frames + 1, off_bytes);
    return CANNY_HIP_OK;
}

// The rule on one host bit map in plain C++: the components of canny_hip_components_from_bits, then the walk of the
// rule from every kept component's first pixel on a byte map with a one-pixel border of zeros.
int canny_hip_contours_from_bits(const unsigned char *bits, int height, int width, int min_area, int *stats,
                                 unsigned long long capacity, unsigned long long *count,
                                 unsigned long long *chain_offsets, int *points, unsigned long long point_capacity,
                                 unsigned long long *point_count)
{
    if (!bits || !count || !point_count || (!chain_offsets && capacity) || (!points && point_capacity))
        return CANNY_HIP_ERR_INVALID;
    int rc = check_contour_dims(height, width, 1);
    if (rc) return rc;
    unsigned long long k = 0;
    if ((rc = canny_hip_components_from_bits(bits, height, width, min_area, nullptr, nullptr, 0, &k))) return rc;
    std::vector<int> rec((size_t)k * CANNY_HIP_CC_STATS);
    if (k && (rc = canny_hip_components_from_bits(bits, height, width, min_area, nullptr, rec.data(), k, &k))) return rc;
    const size_t row_bytes = ((size_t)width + 7) / 8, pitch = (size_t)width + 2;
    std::vector<unsigned char> map(((size_t)height + 2) * pitch, 0);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            map[((size_t)y + 1) * pitch + x + 1] = (bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7))) & 1;
    static const int dy[8] = {0, 1, 1, 1, 0, -1, -1, -1}, dx[8] = {1, 1, 0, -1, -1, -1, 0, 1};
    unsigned long long total = 0;
    if (chain_offsets) chain_offsets[0] = 0;
    for (unsigned long long j = 0; j < k; j++) {
        const int *r = rec.data() + j * CANNY_HIP_CC_STATS;
        const int p0 = r[CANNY_HIP_CC_STAT_FIRST];
        const bool fits = j < capacity;
        auto emit = [&](int px) {
            if (fits && total < point_capacity) points[total] = px;
            total++;
        };
        auto set_at = [&](int y, int x) { return map[((size_t)y + 1) * pitch + x + 1] != 0; };
        int y = p0 / width, x = p0 % width;
        emit(p0);
        int d = -1;
        for (int i = 0; i < 7 && d < 0; i++)
            if (set_at(y + dy[(5 + i) & 7], x + dx[(5 + i) & 7])) d = (5 + i) & 7;
        if (d >= 0) {
            const int q1 = p0 + dy[d] * width + dx[d];
            int cur = p0, s = (d - 1) & 7;
            const unsigned long long cap = 8ull * (unsigned long long)r[CANNY_HIP_CC_STAT_AREA];
            for (unsigned long long step = 0; step < cap; step++) {
                d = -1;
                for (int i = 0; i < 8 && d < 0; i++)
                    if (set_at(y + dy[(s - i) & 7], x + dx[(s - i) & 7])) d = (s - i) & 7;
                if (d < 0) break;
                const int nxt = cur + dy[d] * width + dx[d];
                if (nxt == p0 && cur == q1) break;
                emit(nxt);
                y += dy[d], x += dx[d], cur = nxt, s = (d + 3) & 7;
            }
        }
        if (fits) chain_offsets[j + 1] = total;
    }
    if (stats)
        std::memcpy(stats, rec.data(), (size_t)std::min(k, capacity) * CANNY_HIP_CC_STATS * sizeof(int));
    *count = k;
    *point_count = total;
    return CANNY_HIP_OK;
}

// ---- edge curves -------------------------------------------------------------------------------------
int canny_hip_dev_canny_curves(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, int min_length, int *d_records,
                               unsigned long long capacity, unsigned long long *d_offsets,
                               unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                               unsigned long long *d_point_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CvOut out{d_records, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    if (!d_img || !curve_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames))) return rc;
    return dev_canny_curves(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, min_length, out);
}

int canny_hip_dev_curves_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                              int min_length, int *d_records, unsigned long long capacity, unsigned long long *d_offsets,
                              unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                              unsigned long long *d_point_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CvOut out{d_records, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    if (!d_bits || !curve_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = finish_pending(ctx))) return rc;
    return dev_curves(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), min_length, out);
}

int canny_hip_canny_curves(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int min_length, int *records, unsigned long long capacity,
                           unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                           unsigned long long point_capacity, unsigned long long *point_offsets)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !curve_args_ok(CvOut{records, capacity, offsets, chain_offsets, points, point_capacity, point_offsets}))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames);
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    // a frame has no more than 2 curves and 4 curve points per pixel
    const unsigned long long cap = std::min<unsigned long long>(capacity, 2ull * n);
    const unsigned long long pcap = std::min<unsigned long long>(point_capacity, 4ull * n);
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: offsets | point_offsets | chain_offsets | records | points
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t poff_at = up16(off_bytes), chain_at = up16(poff_at + off_bytes);
    const size_t recs_at = up16(chain_at + ((size_t)cap + 1) * sizeof(unsigned long long));
    const size_t points_at = up16(recs_at + (records ? (size_t)cap * CANNY_HIP_CURVE_RECORD * sizeof(int) : 0));
    HIP_TRY(ctx, ctx->io[1].ensure(points_at + (size_t)pcap * sizeof(int)));
    char *d = (char *)ctx->io[1].p;
    const CvOut out{records && cap ? (int *)(d + recs_at) : nullptr,
                    cap,
                    (unsigned long long *)d,
                    (unsigned long long *)(d + chain_at),
                    pcap ? (int *)(d + points_at) : nullptr,
                    pcap,
                    (unsigned long long *)(d + poff_at)};
    if ((rc = dev_canny_curves(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, n_frames,
                               nullptr, min_length, out)))
        return rc;
    // the offsets come down first: they say how many records and points there are to download
    std::vector<unsigned long long> off(2 * ((size_t)n_frames + 1));
    HIP_TRY(ctx, hipMemcpyAsync(off.data(), out.offsets, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = d2h_sync(ctx, off.data() + n_frames + 1, out.point_offsets, off_bytes))) return rc;
    const unsigned long long n_rec = std::min(off[n_frames], cap);
    if (chain_offsets)
        HIP_TRY(ctx, hipMemcpyAsync(chain_offsets, out.chain_offsets, ((size_t)n_rec + 1) * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec && out.records)
        HIP_TRY(ctx, hipMemcpyAsync(records, out.records, (size_t)n_rec * CANNY_HIP_CURVE_RECORD * sizeof(int),
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_rec && pcap) {
        // chain_offsets is needed on the host to know where the records that fit end
        unsigned long long end = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&end, out.chain_offsets + n_rec, sizeof end, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const unsigned long long n_pts = std::min(end, pcap);
        if (n_pts) {
            HIP_TRY(ctx, hipMemcpyAsync(points, out.points, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    std::memcpy(offsets, off.data(), off_bytes);
    std::memcpy(point_offsets, off.data() + n_frames + 1, off_bytes);
    return CANNY_HIP_OK;
}

// ---- polygon approximation of the chains -------------------------------------------------------------
int canny_hip_dev_polygons_chains(canny_hip_ctx *ctx, const unsigned long long *d_offsets, int n_frames,
                                  unsigned long long capacity, const unsigned long long *d_chain_offsets,
                                  const int *d_points, unsigned long long point_capacity, int width, int height,
                                  unsigned epsilon_q8, unsigned ratio_q16, unsigned long long *d_vertex_offsets,
                                  int *d_vertices, unsigned long long vertex_capacity, long long *d_measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const PgOut out{epsilon_q8, ratio_q16, d_vertex_offsets, d_vertices, vertex_capacity, d_measures};
    if (!d_offsets || n_frames < 1 || !d_chain_offsets || (!d_points && point_capacity) || !polygon_args_ok(out))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_polygon_dims(height, width)) || (rc = finish_pending(ctx))) return rc;
    return dev_polygons(ctx, d_offsets, n_frames, capacity, d_chain_offsets, d_points, point_capacity, width, out);
}

int canny_hip_dev_canny_polygons(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                 int height, int width, int n_frames, short *d_edges, int min_area, int *d_stats,
                                 unsigned long long capacity, unsigned long long *d_offsets,
                                 unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                 unsigned long long *d_point_offsets, unsigned epsilon_q8, unsigned ratio_q16,
                                 unsigned long long *d_vertex_offsets, int *d_vertices, unsigned long long vertex_capacity,
                                 long long *d_measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CtOut ct{d_stats, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    const PgOut out{epsilon_q8, ratio_q16, d_vertex_offsets, d_vertices, vertex_capacity, d_measures};
    if (!d_img || !d_chain_offsets || !contour_args_ok(ct) || !polygon_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = check_polygon_dims(height, width))) return rc;
    return dev_canny_polygons(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, min_area, ct, out);
}

int canny_hip_dev_polygons_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                int min_area, int *d_stats, unsigned long long capacity, unsigned long long *d_offsets,
                                unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                unsigned long long *d_point_offsets, unsigned epsilon_q8, unsigned ratio_q16,
                                unsigned long long *d_vertex_offsets, int *d_vertices, unsigned long long vertex_capacity,
                                long long *d_measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CtOut ct{d_stats, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    const PgOut out{epsilon_q8, ratio_q16, d_vertex_offsets, d_vertices, vertex_capacity, d_measures};
    if (!d_bits || !d_chain_offsets || !contour_args_ok(ct) || !polygon_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = check_polygon_dims(height, width)) ||
        (rc = finish_pending(ctx)))
        return rc;
    if ((rc = dev_contours(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), min_area, ct))) return rc;
    return dev_polygons(ctx, d_offsets, n_frames, capacity, d_chain_offsets, d_points, point_capacity, width, out);
}

int canny_hip_canny_polygons(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                             int max_val, int height, int width, int min_area, int *stats, unsigned long long capacity,
                             unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                             unsigned long long point_capacity, unsigned long long *point_offsets, unsigned epsilon_q8,
                             unsigned ratio_q16, unsigned long long *vertex_offsets, int *vertices,
                             unsigned long long vertex_capacity, long long *measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !offsets || !point_offsets ||
        !polygon_args_ok(PgOut{epsilon_q8, ratio_q16, vertex_offsets, vertices, vertex_capacity, measures}))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = check_polygon_dims(height, width))) return rc;
    const size_t n = npx(height, width, n_frames);
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    // a frame has no more records than pixels, no more chain points than 8 per pixel and one per record, and a polygon no
    // more vertices than its chain has points.  point_capacity itself decides which chains are complete, so it is
    // clamped only where that changes nothing: every chain ends at or below 9 n.
    const unsigned long long cap = std::min<unsigned long long>(capacity, n);
    const unsigned long long pcap = std::min<unsigned long long>(point_capacity, 9ull * n);
    const unsigned long long vcap = std::min<unsigned long long>(vertex_capacity, pcap);
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: offsets | point_offsets | chain_offsets | vertex_offsets | measures | stats | vertices; the chain
    // points in a block of their own, which never crosses to the host when points == NULL
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t csr_bytes = ((size_t)cap + 1) * sizeof(unsigned long long);
    const size_t poff_at = up16(off_bytes), chain_at = up16(poff_at + off_bytes), voff_at = up16(chain_at + csr_bytes);
    const size_t meas_at = up16(voff_at + csr_bytes);
    const size_t stats_at = up16(meas_at + (measures ? (size_t)cap * 4 * sizeof(long long) : 0));
    const size_t verts_at = up16(stats_at + (stats ? (size_t)cap * CANNY_HIP_CC_STATS * sizeof(int) : 0));
    HIP_TRY(ctx, ctx->io[1].ensure(verts_at + (size_t)vcap * sizeof(int)));
    HIP_TRY(ctx, ctx->pg_points.ensure((size_t)pcap * sizeof(int) + 16));
    char *d = (char *)ctx->io[1].p;
    const CtOut ct{stats && cap ? (int *)(d + stats_at) : nullptr,
                   cap,
                   (unsigned long long *)d,
                   (unsigned long long *)(d + chain_at),
                   pcap ? (int *)ctx->pg_points.p : nullptr,
                   pcap,
                   (unsigned long long *)(d + poff_at)};
    const PgOut out{epsilon_q8,
                    ratio_q16,
                    (unsigned long long *)(d + voff_at),
                    vcap ? (int *)(d + verts_at) : nullptr,
                    vcap,
                    measures && cap ? (long long *)(d + meas_at) : nullptr};
    if ((rc = dev_canny_polygons(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, n_frames,
                                 nullptr, min_area, ct, out)))
        return rc;
    // the offsets come down first: they say how many records there are to download
    std::vector<unsigned long long> off(2 * ((size_t)n_frames + 1));
    HIP_TRY(ctx, hipMemcpyAsync(off.data(), ct.offsets, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = d2h_sync(ctx, off.data() + n_frames + 1, ct.point_offsets, off_bytes))) return rc;
    const unsigned long long n_rec = std::min(off[n_frames], cap);
    unsigned long long ends[2] = {0, 0}; // where the stored chains and the polygons end
    HIP_TRY(ctx, hipMemcpyAsync(&ends[0], ct.chain_offsets + n_rec, sizeof ends[0], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[1], out.vertex_offsets + n_rec, sizeof ends[1], hipMemcpyDeviceToHost, ctx->stream));
    if (chain_offsets)
        HIP_TRY(ctx, hipMemcpyAsync(chain_offsets, ct.chain_offsets, ((size_t)n_rec + 1) * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(vertex_offsets, out.vertex_offsets, ((size_t)n_rec + 1) * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec && ct.stats)
        HIP_TRY(ctx, hipMemcpyAsync(stats, ct.stats, (size_t)n_rec * CANNY_HIP_CC_STATS * sizeof(int),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec && out.measures)
        HIP_TRY(ctx, hipMemcpyAsync(measures, out.measures, (size_t)n_rec * 4 * sizeof(long long), hipMemcpyDeviceToHost,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long n_pts = points ? std::min(ends[0], pcap) : 0, n_verts = std::min(ends[1], vcap);
    if (n_pts) HIP_TRY(ctx, hipMemcpyAsync(points, ct.points, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (n_verts)
        HIP_TRY(ctx, hipMemcpyAsync(vertices, out.vertices, (size_t)n_verts * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(offsets, off.data(), off_bytes);
    std::memcpy(point_offsets, off.data() + n_frames + 1, off_bytes);
    return CANNY_HIP_OK;
}

// canny_hip_polygons_from_chains, the rule in plain C++, lives in canny_polygons_host.cpp: it needs no HIP.

// ---- contour shape measures ---------------------------------------------------------------------------
int canny_hip_dev_shapes_chains(canny_hip_ctx *ctx, const unsigned long long *d_offsets, int n_frames,
                                unsigned long long capacity, const unsigned long long *d_chain_offsets, const int *d_points,
                                unsigned long long point_capacity, int width, int height,
                                unsigned long long *d_hull_offsets, int *d_hull, unsigned long long hull_capacity,
                                long long *d_measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const ShOut out{d_hull_offsets, d_hull, hull_capacity, d_measures};
    if (!d_offsets || n_frames < 1 || !d_chain_offsets || (!d_points && point_capacity) || !shape_args_ok(out))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_shape_dims(height, width)) || (rc = finish_pending(ctx))) return rc;
    return dev_shapes(ctx, d_offsets, n_frames, capacity, d_chain_offsets, d_points, point_capacity, width, out);
}

int canny_hip_dev_canny_shapes(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, int min_area, int *d_stats,
                               unsigned long long capacity, unsigned long long *d_offsets,
                               unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                               unsigned long long *d_point_offsets, unsigned long long *d_hull_offsets, int *d_hull,
                               unsigned long long hull_capacity, long long *d_measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CtOut ct{d_stats, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    const ShOut out{d_hull_offsets, d_hull, hull_capacity, d_measures};
    if (!d_img || !d_chain_offsets || !contour_args_ok(ct) || !shape_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = check_shape_dims(height, width))) return rc;
    return dev_canny_shapes(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, min_area, ct, out);
}

int canny_hip_dev_shapes_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                              int min_area, int *d_stats, unsigned long long capacity, unsigned long long *d_offsets,
                              unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                              unsigned long long *d_point_offsets, unsigned long long *d_hull_offsets, int *d_hull,
                              unsigned long long hull_capacity, long long *d_measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CtOut ct{d_stats, capacity, d_offsets, d_chain_offsets, d_points, point_capacity, d_point_offsets};
    const ShOut out{d_hull_offsets, d_hull, hull_capacity, d_measures};
    if (!d_bits || !d_chain_offsets || !contour_args_ok(ct) || !shape_args_ok(out)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = check_shape_dims(height, width)) ||
        (rc = finish_pending(ctx)))
        return rc;
    if ((rc = dev_contours(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), min_area, ct))) return rc;
    return dev_shapes(ctx, d_offsets, n_frames, capacity, d_chain_offsets, d_points, point_capacity, width, out);
}

int canny_hip_canny_shapes(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int min_area, int *stats, unsigned long long capacity,
                           unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                           unsigned long long point_capacity, unsigned long long *point_offsets,
                           unsigned long long *hull_offsets, int *hull, unsigned long long hull_capacity,
                           long long *measures)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !offsets || !point_offsets || !shape_args_ok(ShOut{hull_offsets, hull, hull_capacity, measures}))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = check_contour_dims(height, width, n_frames)) || (rc = check_shape_dims(height, width))) return rc;
    const size_t n = npx(height, width, n_frames);
    const size_t off_bytes = ((size_t)n_frames + 1) * sizeof(unsigned long long);
    // the clamps of canny_hip_canny_polygons: a hull has no more vertices than its chain has points
    const unsigned long long cap = std::min<unsigned long long>(capacity, n);
    const unsigned long long pcap = std::min<unsigned long long>(point_capacity, 9ull * n);
    const unsigned long long hcap = std::min<unsigned long long>(hull_capacity, pcap);
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: offsets | point_offsets | chain_offsets | hull_offsets | measures | stats | hull; the chain points
    // in a block of their own, which never crosses to the host when points == NULL
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t csr_bytes = ((size_t)cap + 1) * sizeof(unsigned long long);
    const size_t poff_at = up16(off_bytes), chain_at = up16(poff_at + off_bytes), hoff_at = up16(chain_at + csr_bytes);
    const size_t meas_at = up16(hoff_at + csr_bytes);
    const size_t stats_at = up16(meas_at + (measures ? (size_t)cap * CANNY_HIP_SHAPE_WORDS * sizeof(long long) : 0));
    const size_t hull_at = up16(stats_at + (stats ? (size_t)cap * CANNY_HIP_CC_STATS * sizeof(int) : 0));
    HIP_TRY(ctx, ctx->io[1].ensure(hull_at + (size_t)hcap * sizeof(int)));
    HIP_TRY(ctx, ctx->pg_points.ensure((size_t)pcap * sizeof(int) + 16));
    char *d = (char *)ctx->io[1].p;
    const CtOut ct{stats && cap ? (int *)(d + stats_at) : nullptr,
                   cap,
                   (unsigned long long *)d,
                   (unsigned long long *)(d + chain_at),
                   pcap ? (int *)ctx->pg_points.p : nullptr,
                   pcap,
                   (unsigned long long *)(d + poff_at)};
    const ShOut out{(unsigned long long *)(d + hoff_at), hcap ? (int *)(d + hull_at) : nullptr, hcap,
                    measures && cap ? (long long *)(d + meas_at) : nullptr};
    if ((rc = dev_canny_shapes(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, n_frames,
                               nullptr, min_area, ct, out)))
        return rc;
    // the offsets come down first: they say how many records there are to download
    std::vector<unsigned long long> off(2 * ((size_t)n_frames + 1));
    HIP_TRY(ctx, hipMemcpyAsync(off.data(), ct.offsets, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = d2h_sync(ctx, off.data() + n_frames + 1, ct.point_offsets, off_bytes))) return rc;
    const unsigned long long n_rec = std::min(off[n_frames], cap);
    unsigned long long ends[2] = {0, 0}; // where the stored chains and the hulls end
    HIP_TRY(ctx, hipMemcpyAsync(&ends[0], ct.chain_offsets + n_rec, sizeof ends[0], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[1], out.hull_offsets + n_rec, sizeof ends[1], hipMemcpyDeviceToHost, ctx->stream));
    if (chain_offsets)
        HIP_TRY(ctx, hipMemcpyAsync(chain_offsets, ct.chain_offsets, ((size_t)n_rec + 1) * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hull_offsets, out.hull_offsets, ((size_t)n_rec + 1) * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec && ct.stats)
        HIP_TRY(ctx, hipMemcpyAsync(stats, ct.stats, (size_t)n_rec * CANNY_HIP_CC_STATS * sizeof(int),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec && out.measures)
        HIP_TRY(ctx, hipMemcpyAsync(measures, out.measures, (size_t)n_rec * CANNY_HIP_SHAPE_WORDS * sizeof(long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long n_pts = points ? std::min(ends[0], pcap) : 0, n_hull = std::min(ends[1], hcap);
    if (n_pts) HIP_TRY(ctx, hipMemcpyAsync(points, ct.points, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (n_hull) HIP_TRY(ctx, hipMemcpyAsync(hull, out.hull, (size_t)n_hull * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(offsets, off.data(), off_bytes);
    std::memcpy(point_offsets, off.data() + n_frames + 1, off_bytes);
    return CANNY_HIP_OK;
}

// canny_hip_shapes_from_chains, the rule in plain C++, lives in canny_shapes_host.cpp: it needs no HIP.

// ---- Euclidean distance transform -------------------------------------------------------------------
int canny_hip_dev_canny_edt(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                            int height, int width, int n_frames, short *d_edges, int *d_dist2, float *d_dist,
                            int *d_nearest)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || (!d_dist2 && !d_dist && !d_nearest)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_edt_dims(height, width, n_frames))) return rc;
    return dev_canny_edt(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges,
                         EdtOut{d_dist2, d_dist, d_nearest});
}

int canny_hip_dev_edt_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                           int *d_dist2, float *d_dist, int *d_nearest)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || (!d_dist2 && !d_dist && !d_nearest)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_edt_dims(height, width, n_frames)) || (rc = finish_pending(ctx))) return rc;
    return dev_edt(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), EdtOut{d_dist2, d_dist, d_nearest});
}

int canny_hip_canny_edt(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                        int height, int width, int *dist2, float *dist, int *nearest)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || (!dist2 && !dist && !nearest)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_edt_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames);
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block per plane asked for
    void *host[3] = {dist2, dist, nearest};
    void *dev[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; k++) {
        if (!host[k]) continue;
        HIP_TRY(ctx, ctx->io[1 + k].ensure(n * 4));
        dev[k] = ctx->io[1 + k].p;
    }
    if ((rc = dev_canny_edt(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, n_frames,
                            nullptr, EdtOut{(int *)dev[0], (float *)dev[1], (int *)dev[2]})))
        return rc;
    for (int k = 0; k < 3; k++)
        if (host[k]) HIP_TRY(ctx, hipMemcpyAsync(host[k], dev[k], n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

// The rule on one host bit map, the two passes of canny_edt.hip in plain C++: per row the column of the nearest set pixel
// (ties to the left), then per column the lower envelope of the rows' parabolas with a strict pop (ties to the smaller row).
int canny_hip_edt_from_bits(const unsigned char *bits, int height, int width, int *dist2, float *dist, int *nearest)
{
    if (!bits || (!dist2 && !dist && !nearest)) return CANNY_HIP_ERR_INVALID;
    int rc = check_edt_dims(height, width, 1);
    if (rc) return rc;
    const size_t row_bytes = ((size_t)width + 7) / 8, n = (size_t)height * width;
    constexpr int kNone = -1;
    std::vector<int> col(n); // column of the nearest set pixel of the row, kNone if the row has none
    for (int y = 0; y < height; y++) {
        const unsigned char *row = bits + (size_t)y * row_bytes;
        int *g = col.data() + (size_t)y * width;
        int last = kNone;
        for (int x = 0; x < width; x++) {
            if ((row[x >> 3] >> (7 - (x & 7))) & 1) last = x;
            g[x] = last;
        }
        int next = kNone;
        for (int x = width - 1; x >= 0; x--) {
            if (g[x] == x) next = x;
            if (next != kNone && (g[x] == kNone || next - x < x - g[x])) g[x] = next; // strictly nearer: ties stay left
        }
    }
    std::vector<int> s(height), t(height);
    for (int c = 0; c < width; c++) {
        auto G = [&](int r) { return col[(size_t)r * width + c]; };
        auto f = [&](int x, int r) {
            const long long dx = x - r, hx = c - G(r);
            return dx * dx + hx * hx;
        };
        int q = -1;
        for (int u = 0; u < height; u++) {
            if (G(u) == kNone) continue;
            while (q >= 0 && f(t[q], s[q]) > f(t[q], u)) q--;
            if (q < 0) {
                q = 0, s[0] = u, t[0] = 0;
                continue;
            }
            const long long i = s[q], hu = c - G(u), hi = c - G((int)i);
            const long long sep = ((long long)u * u - i * i + hu * hu - hi * hi) / (2 * (u - i)) + 1; // numerator >= 0
            if (sep < height) q++, s[q] = u, t[q] = (int)sep;
        }
        for (int x = height - 1; x >= 0; x--) {
            const size_t o = (size_t)x * width + c;
            if (q < 0) {
                if (dist2) dist2[o] = CANNY_HIP_EDT_NONE;
                if (dist) dist[o] = INFINITY;
                if (nearest) nearest[o] = -1;
                continue;
            }
            while (x < t[q]) q--;
            const int d2 = (int)f(x, s[q]);
            if (dist2) dist2[o] = d2;
            if (dist) dist[o] = (float)std::sqrt((double)d2);
            if (nearest) nearest[o] = s[q] * width + G(s[q]);
        }
    }
    return CANNY_HIP_OK;
}

// ---- profiling --------------------------------------------------------------------------------------
int canny_hip_profile_enable(canny_hip_ctx *ctx, int on)
{
    if (!ctx) return CANNY_HIP_ERR_INVALID;
    ctx->prof = on != 0;
    return CANNY_HIP_OK;
}

static int profile_collect(canny_hip_ctx *ctx)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < canny_hip_ctx::kProfSlots; s++) {
        for (auto &e : ctx->pending[s]) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
                ctx->total_ms[s] += ms;
                ctx->launches[s] += 1;
            } else {
                (void)hipGetLastError();
            }
            ctx->pool.push_back(e);
        }
        ctx->pending[s].clear();
    }
    return CANNY_HIP_OK;
}

int canny_hip_profile_reset(canny_hip_ctx *ctx)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = profile_collect(ctx))) return rc;
    for (int s = 0; s < canny_hip_ctx::kProfSlots; s++) {
        ctx->total_ms[s] = 0.0;
        ctx->launches[s] = 0;
    }
    return CANNY_HIP_OK;
}

int canny_hip_profile_get(canny_hip_ctx *ctx, int stage, double *total_ms, long *launches)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (stage < 0 || stage >= CANNY_HIP_STAGE_END || !total_ms || !launches) return CANNY_HIP_ERR_INVALID;
    if ((rc = profile_collect(ctx))) return rc;
    *total_ms = ctx->total_ms[stage];
    *launches = ctx->launches[stage];
    return CANNY_HIP_OK;
}

// ---- Hough lines ----------------------------------------------------------------------------------------
int canny_hip_hough_geometry(int height, int width, float rho, float theta, float min_theta, float max_theta,
                             int *numangle, int *numrho)
{
    if (!numangle || !numrho) return CANNY_HIP_ERR_INVALID;
    return hough_geometry(height, width, rho, theta, min_theta, max_theta, numangle, numrho);
}

int canny_hip_hough_tables(float rho, float theta, float min_theta, int numangle, float *tab_cos, float *tab_sin)
{
    if (!tab_cos || !tab_sin || numangle < 1 || !std::isfinite(rho) || !std::isfinite(theta) ||
        !std::isfinite(min_theta) || rho <= 0.0f || theta <= 0.0f || min_theta < 0.0f || min_theta >= (float)M_PI)
        return CANNY_HIP_ERR_INVALID;
    hough_tables(rho, theta, min_theta, numangle, tab_cos, tab_sin);
    return CANNY_HIP_OK;
}

int canny_hip_hough_line_of(unsigned int base, int numrho, float rho, float theta, float min_theta, float *line_rho,
                            float *line_theta)
{
    if (!line_rho || !line_theta || numrho < 1 || numrho > 0x7ffffff0 || !std::isfinite(rho) || !std::isfinite(theta) ||
        !std::isfinite(min_theta) || rho <= 0.0f || theta <= 0.0f)
        return CANNY_HIP_ERR_INVALID;
    const unsigned stride = (unsigned)numrho + 2u;
    const int n = (int)(base / stride) - 1, r = (int)(base % stride) - 1;
    const float centre = (float)(numrho - 1) * 0.5f;
    const float d = (float)r - centre; // each operation rounded on its own (-ffp-contract=off)
    const float t = (float)n * theta;
    *line_rho = d * rho;
    *line_theta = min_theta + t;
    return CANNY_HIP_OK;
}

int canny_hip_dev_hough_points(canny_hip_ctx *ctx, const unsigned int *d_points, const unsigned long long *d_offsets,
                               int n_frames, int height, int width, float rho, float theta, int threshold, int lines_max,
                               float min_theta, float max_theta, float *d_lines, int *d_votes, unsigned int *d_bases,
                               int *d_counts, int *d_accum)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_points || !d_offsets) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const HoughOut out{d_lines, d_votes, d_bases, d_counts, d_accum};
    HoughGeom hg;
    int lds_rows = 0;
    if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, out, hg, &lds_rows)) ||
        (rc = finish_pending(ctx)))
        return rc;
    return dev_hough(ctx, nullptr, nullptr, d_points, d_offsets, make_hyst_geom(height, width, n_frames), hg, lds_rows,
                     threshold, lines_max, out);
}

int canny_hip_dev_hough_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int height, int width,
                             float rho, float theta, int threshold, int lines_max, float min_theta, float max_theta,
                             float *d_lines, int *d_votes, unsigned int *d_bases, int *d_counts, int *d_accum)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const HoughOut out{d_lines, d_votes, d_bases, d_counts, d_accum};
    HoughGeom hg;
    int lds_rows = 0;
    if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, out, hg, &lds_rows)) ||
        (rc = finish_pending(ctx)))
        return rc;
    return dev_hough(ctx, nullptr, d_bits, nullptr, nullptr, make_hyst_geom(height, width, n_frames), hg, lds_rows,
                     threshold, lines_max, out);
}

int canny_hip_dev_canny_hough(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                              int height, int width, int n_frames, short *d_edges, float rho, float theta, int threshold,
                              int lines_max, float min_theta, float max_theta, float *d_lines, int *d_votes,
                              unsigned int *d_bases, int *d_counts, int *d_accum)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const HoughOut out{d_lines, d_votes, d_bases, d_counts, d_accum};
    HoughGeom hg;
    int lds_rows = 0;
    if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, out, hg, &lds_rows)))
        return rc;
    const uint64_t *strong;
    if ((rc = dev_canny_map(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, &strong))) return rc;
    return dev_hough(ctx, strong, nullptr, nullptr, nullptr, make_hyst_geom(height, width, n_frames), hg, lds_rows,
                     threshold, lines_max, out);
}

int canny_hip_canny_hough(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                          int max_val, int height, int width, float rho, float theta, int threshold, int lines_max,
                          float min_theta, float max_theta, float *lines, int *votes, unsigned int *bases, int *counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !counts) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    HoughGeom hg;
    int lds_rows = 0;
    {
        const HoughOut probe{nullptr, nullptr, nullptr, counts, nullptr};
        if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, probe, hg, &lds_rows)))
            return rc;
    }
    const size_t slots = (size_t)n_frames * lines_max;
    // one staging block: lines (2 floats per slot) | votes | bases | counts
    HIP_TRY(ctx, ctx->io[1].ensure(slots * 16 + (size_t)n_frames * sizeof(int)));
    char *d = (char *)ctx->io[1].p;
    const HoughOut out{lines ? (float *)d : nullptr, votes ? (int *)(d + slots * 8) : nullptr,
                       bases ? (unsigned *)(d + slots * 12) : nullptr, (int *)(d + slots * 16), nullptr};
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_hough(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                        n_frames, nullptr, rho, theta, threshold, lines_max, min_theta, max_theta,
                                        out.d_lines, out.d_votes, out.d_bases, out.d_counts, nullptr)))
        return rc;
    std::vector<int> cnt((size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), out.d_counts, cnt.size() * sizeof(int)))) return rc;
    // only the lines come down: the filled slots of each frame, nothing of the accumulators
    for (int f = 0; f < n_frames; f++) {
        const size_t k = (size_t)std::min(cnt[f], lines_max), at = (size_t)f * lines_max;
        if (!k) continue;
        if (lines)
            HIP_TRY(ctx, hipMemcpyAsync(lines + 2 * at, out.d_lines + 2 * at, k * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (votes) HIP_TRY(ctx, hipMemcpyAsync(votes + at, out.d_votes + at, k * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (bases) HIP_TRY(ctx, hipMemcpyAsync(bases + at, out.d_bases + at, k * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(counts, cnt.data(), cnt.size() * sizeof(int));
    return CANNY_HIP_OK;
}

// ---- Hough line segments ------------------------------------------------------------------------------------
int canny_hip_hough_segments_from_bits(const unsigned char *bits, int height, int width, float rho, float theta,
                                       float min_theta, float max_theta, const unsigned int *bases, int n_lines,
                                       int min_length, int max_gap, int exclusive, int *segments, int segments_max,
                                       int *count)
{
    if (!bits || !segments || !count || n_lines < 0 || (n_lines && !bases)) return CANNY_HIP_ERR_INVALID;
    int rc = check_dims(height, width, 1);
    if (rc) return rc;
    const SegArgs a{min_length, max_gap, exclusive, segments_max};
    int numangle, numrho;
    if ((rc = hough_geometry(height, width, rho, theta, min_theta, max_theta, &numangle, &numrho))) return rc;
    if ((rc = segments_check(height, width, 1, n_lines, a, false))) return rc;
    std::vector<float> tab(2 * (size_t)numangle);
    hough_tables(rho, theta, min_theta, numangle, tab.data(), tab.data() + numangle);
    // the working map W as the list of its set pixels
    const size_t row_bytes = ((size_t)width + 7) / 8;
    std::vector<int> px, py;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            if (bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7)) & 1) px.push_back(x), py.push_back(y);
    std::vector<char> alive(px.size(), 1);
    const int half = (numrho - 1) / 2, axis = std::max(height, width);
    std::vector<int> cnt((size_t)axis), lo((size_t)axis);
    std::vector<char> keep((size_t)axis);
    std::vector<size_t> members;
    const unsigned stride = (unsigned)numrho + 2u;
    int total = 0;
    for (int k = 0; k < n_lines; k++) {
        const int n = (int)(bases[k] / stride) - 1, r = (int)(bases[k] % stride) - 1;
        if (n < 0 || n >= numangle || r < 0 || r >= numrho) continue; // not a line
        const float c = tab[n], s = tab[(size_t)numangle + n];
        const bool major_x = std::fabs(s) >= std::fabs(c);
        const int L = major_x ? width : height;
        std::fill(cnt.begin(), cnt.begin() + L, 0);
        std::fill(keep.begin(), keep.begin() + L, 0);
        members.clear();
        for (size_t i = 0; i < px.size(); i++) { // the support: every pixel of W that votes for the cell
            if (!alive[i] || host_vote_r(px[i], py[i], c, s, half) != r) continue;
            const int t = major_x ? px[i] : py[i], m = major_x ? py[i] : px[i];
            if (!cnt[t] || m < lo[t]) lo[t] = m;
            cnt[t]++;
            members.push_back(i);
        }
        int ta = -1, last = -1, support = 0;
        auto close = [&]() {
            if (last - ta < min_length) return;
            if (total < segments_max) {
                int *rec = segments + (size_t)total * CANNY_HIP_SEGMENT_INTS;
                rec[0] = major_x ? ta : lo[ta], rec[1] = major_x ? lo[ta] : ta;
                rec[2] = major_x ? last : lo[last], rec[3] = major_x ? lo[last] : last;
                rec[4] = k, rec[5] = support;
            }
            total++;
            std::fill(keep.begin() + ta, keep.begin() + last + 1, 1);
        };
        for (int t = 0; t < L; t++) {
            if (!cnt[t]) continue;
            if (ta >= 0 && t - last - 1 > max_gap) close(), ta = -1;
            if (ta < 0) ta = t, support = 0;
            support += cnt[t];
            last = t;
        }
        if (ta >= 0) close();
        if (exclusive)
            for (size_t i : members)
                if (keep[major_x ? px[i] : py[i]]) alive[i] = 0;
    }
    *count = total;
    return CANNY_HIP_OK;
}

int canny_hip_dev_hough_segments_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int height, int width,
                                      float rho, float theta, float min_theta, float max_theta,
                                      const unsigned int *d_bases, const int *d_line_counts, int lines_max, int min_length,
                                      int max_gap, int exclusive, int *d_segments, int segments_max, int *d_seg_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_bases || !d_line_counts || !d_segments || !d_seg_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const SegArgs a{min_length, max_gap, exclusive, segments_max};
    HoughGeom hg;
    if ((rc = hough_geometry(height, width, rho, theta, min_theta, max_theta, &hg.numangle, &hg.numrho))) return rc;
    if (lines_max > kHoughMaxLines) return CANNY_HIP_ERR_UNSUPPORTED;
    if ((rc = segments_check(height, width, n_frames, lines_max, a, true))) return rc;
    hg.rho = rho, hg.theta = theta, hg.min_theta = min_theta;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_segments(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), hg, d_bases, d_line_counts,
                        lines_max, a, d_segments, d_seg_counts);
}

int canny_hip_dev_canny_hough_segments(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                       int max_val, int height, int width, int n_frames, short *d_edges, float rho,
                                       float theta, int threshold, int lines_max, float min_theta, float max_theta,
                                       float *d_lines, int *d_votes, unsigned int *d_bases, int *d_line_counts,
                                       int *d_accum, int min_length, int max_gap, int exclusive, int *d_segments,
                                       int segments_max, int *d_seg_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_segments || !d_seg_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const SegArgs a{min_length, max_gap, exclusive, segments_max};
    HoughGeom hg;
    {
        int lds_rows = 0, probe = 0;
        const HoughOut out{nullptr, nullptr, nullptr, &probe, nullptr};
        if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, out, hg, &lds_rows)))
            return rc;
    }
    if ((rc = segments_check(height, width, n_frames, lines_max, a, true))) return rc;
    // bases and line counts the caller does not want live in the context: line counts | bases
    const size_t slots = (size_t)n_frames * lines_max;
    if (!d_bases || !d_line_counts) {
        HIP_TRY(ctx, ctx->seg_lines.ensure((slots + (size_t)n_frames) * sizeof(int)));
        int *own = (int *)ctx->seg_lines.p;
        if (!d_bases) d_bases = (unsigned int *)own;
        if (!d_line_counts) d_line_counts = own + slots;
    }
    if ((rc = canny_hip_dev_canny_hough(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, rho, theta,
                                        threshold, lines_max, min_theta, max_theta, d_lines, d_votes, d_bases,
                                        d_line_counts, d_accum)))
        return rc;
    // the segments follow the MAP: max_val > 255 zeroes every reached pixel although strong bits are set
    const uint64_t *strong = max_val > 255 ? nullptr : (const uint64_t *)ctx->plane_s.p;
    return dev_segments(ctx, strong, nullptr, make_hyst_geom(height, width, n_frames), hg, d_bases, d_line_counts,
                        lines_max, a, d_segments, d_seg_counts);
}

int canny_hip_canny_hough_segments(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                   int max_val, int height, int width, float rho, float theta, int threshold,
                                   int lines_max, float min_theta, float max_theta, int min_length, int max_gap,
                                   int exclusive, float *lines, int *votes, unsigned int *bases, int *line_counts,
                                   int *segments, int segments_max, int *seg_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !segments || !seg_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    {
        const SegArgs a{min_length, max_gap, exclusive, segments_max};
        HoughGeom hg;
        int lds_rows = 0, probe = 0;
        const HoughOut out{nullptr, nullptr, nullptr, &probe, nullptr};
        if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, out, hg, &lds_rows)) ||
            (rc = segments_check(height, width, n_frames, lines_max, a, true)))
            return rc;
    }
    const size_t slots = (size_t)n_frames * lines_max, seg_ints = (size_t)n_frames * segments_max * CANNY_HIP_SEGMENT_INTS;
    // staging: lines (2 floats per slot) | votes | bases | line counts | segment counts; the records in a block of their own
    HIP_TRY(ctx, ctx->io[1].ensure(slots * 16 + 2 * (size_t)n_frames * sizeof(int)));
    HIP_TRY(ctx, ctx->io[2].ensure(seg_ints * sizeof(int)));
    char *d = (char *)ctx->io[1].p;
    float *d_lines = (float *)d;
    int *d_votes = (int *)(d + slots * 8);
    unsigned *d_bases = (unsigned *)(d + slots * 12);
    int *d_line_counts = (int *)(d + slots * 16), *d_seg_counts = d_line_counts + n_frames;
    int *d_segments = (int *)ctx->io[2].p;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_hough_segments(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height,
                                                 width, n_frames, nullptr, rho, theta, threshold, lines_max, min_theta,
                                                 max_theta, lines ? d_lines : nullptr, votes ? d_votes : nullptr, d_bases,
                                                 d_line_counts, nullptr, min_length, max_gap, exclusive, d_segments,
                                                 segments_max, d_seg_counts)))
        return rc;
    std::vector<int> cnt(2 * (size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_line_counts, cnt.size() * sizeof(int)))) return rc;
    // the counts first, then only the filled slots of each frame
    for (int f = 0; f < n_frames; f++) {
        const size_t k = (size_t)std::min(cnt[f], lines_max), at = (size_t)f * lines_max;
        if (k && lines)
            HIP_TRY(ctx, hipMemcpyAsync(lines + 2 * at, d_lines + 2 * at, k * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (k && votes) HIP_TRY(ctx, hipMemcpyAsync(votes + at, d_votes + at, k * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (k && bases) HIP_TRY(ctx, hipMemcpyAsync(bases + at, d_bases + at, k * 4, hipMemcpyDeviceToHost, ctx->stream));
        const size_t j = (size_t)std::min(cnt[(size_t)n_frames + f], segments_max);
        const size_t sat = (size_t)f * segments_max * CANNY_HIP_SEGMENT_INTS;
        if (j)
            HIP_TRY(ctx, hipMemcpyAsync(segments + sat, d_segments + sat, j * CANNY_HIP_SEGMENT_INTS * sizeof(int),
                                        hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (line_counts) std::memcpy(line_counts, cnt.data(), (size_t)n_frames * sizeof(int));
    std::memcpy(seg_counts, cnt.data() + n_frames, (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

// ---- sub-pixel line fits (canny_line_fits.hip) ------------------------------------
namespace {

// THE check of the fit arguments; needs no device and writes nothing
int line_fits_check(int height, int width, int n_frames, float rho, int segments_max, int options, const int *d_fits)
{
    if ((options & ~(CANNY_HIP_LINE_FIT_GATE | CANNY_HIP_LINE_FIT_REFINED_ONLY)) || !d_fits || ((uintptr_t)d_fits & 15) ||
        segments_max < 1 || height < 2 || width < 2)
        return CANNY_HIP_ERR_INVALID;
    if (std::max(height, width) > CANNY_HIP_LINE_FIT_MAX_AXIS || rho > CANNY_HIP_LINE_FIT_MAX_RHO)
        return CANNY_HIP_ERR_UNSUPPORTED;
    if ((double)n_frames * (double)segments_max * CANNY_HIP_LINE_FIT_INTS >= 2147483648.0) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// the fits of the segment records in d_segments, queued on the context's stream
int dev_line_fits(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const HoughGeom &hg,
                  const unsigned *d_bases, const int *d_line_counts, int lines_max, const int *d_segments,
                  const int *d_seg_counts, int segments_max, const void *d_plane, bool plane_u8, int options, int *d_fits)
{
    int rc = hough_tab_ensure(ctx, hg);
    if (rc) return rc;
    const SegGeom sg{hg.numangle, hg.numrho, hough_segments_halfwin(g.height, g.width, hg.rho), 0, 0, lines_max,
                     segments_max};
    StageTimer tm(ctx, canny_hip_ctx::kProfLineFits + CANNY_HIP_LINE_FIT_PART_FIT);
    HIP_TRY(ctx, launch_line_fits(strong, bits, g, sg, (const float *)ctx->hough_tab.p, d_bases, d_line_counts, d_segments,
                                  d_seg_counts, d_plane, plane_u8, options, d_fits, ctx->stream));
    return CANNY_HIP_OK;
}

} // namespace

int canny_hip_dev_line_fits_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, const void *d_plane, int plane_is_u8,
                                 int n_frames, int height, int width, float rho, float theta, float min_theta,
                                 float max_theta, const unsigned int *d_bases, const int *d_line_counts, int lines_max,
                                 const int *d_segments, const int *d_seg_counts, int segments_max, int options,
                                 int *d_fits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_bases || !d_line_counts || !d_segments || !d_seg_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    HoughGeom hg;
    if ((rc = hough_geometry(height, width, rho, theta, min_theta, max_theta, &hg.numangle, &hg.numrho))) return rc;
    if (lines_max > kHoughMaxLines) return CANNY_HIP_ERR_UNSUPPORTED;
    if ((rc = line_fits_check(height, width, n_frames, rho, segments_max, options, d_fits))) return rc;
    hg.rho = rho, hg.theta = theta, hg.min_theta = min_theta;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, height, width) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        d_plane = ctx->smoothed.p;
        plane_is_u8 = ctx->last_canny_u8;
    }
    if ((rc = finish_pending(ctx))) return rc;
    return dev_line_fits(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), hg, d_bases, d_line_counts,
                         lines_max, d_segments, d_seg_counts, segments_max, d_plane, plane_is_u8 != 0, options, d_fits);
}

int canny_hip_dev_canny_hough_line_fits(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                        int max_val, int height, int width, int n_frames, short *d_edges, float rho,
                                        float theta, int threshold, int lines_max, float min_theta, float max_theta,
                                        float *d_lines, int *d_votes, unsigned int *d_bases, int *d_line_counts,
                                        int *d_accum, int min_length, int max_gap, int exclusive, int *d_segments,
                                        int segments_max, int *d_seg_counts, int options, int *d_fits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img || !d_segments || !d_seg_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    HoughGeom hg;
    if ((rc = hough_geometry(height, width, rho, theta, min_theta, max_theta, &hg.numangle, &hg.numrho))) return rc;
    if ((rc = line_fits_check(height, width, n_frames, rho, segments_max, options, d_fits))) return rc;
    hg.rho = rho, hg.theta = theta, hg.min_theta = min_theta;
    // the fits need the bases and the line counts: the context's own where the caller wants none (as the segments do)
    const size_t slots = (size_t)n_frames * lines_max;
    if (!d_bases || !d_line_counts) {
        HIP_TRY(ctx, ctx->seg_lines.ensure((slots + (size_t)n_frames) * sizeof(int)));
        int *own = (int *)ctx->seg_lines.p;
        if (!d_bases) d_bases = (unsigned int *)own;
        if (!d_line_counts) d_line_counts = own + slots;
    }
    if ((rc = canny_hip_dev_canny_hough_segments(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, rho,
                                                 theta, threshold, lines_max, min_theta, max_theta, d_lines, d_votes,
                                                 d_bases, d_line_counts, d_accum, min_length, max_gap, exclusive,
                                                 d_segments, segments_max, d_seg_counts)))
        return rc;
    if (max_val > 255) return CANNY_HIP_OK; // the empty map: every segment count is 0
    return dev_line_fits(ctx, (const uint64_t *)ctx->plane_s.p, nullptr, make_hyst_geom(height, width, n_frames), hg,
                         d_bases, d_line_counts, lines_max, d_segments, d_seg_counts, segments_max, ctx->smoothed.p,
                         ctx->last_canny_u8 != 0, options, d_fits);
}

int canny_hip_canny_hough_line_fits(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                    int max_val, int height, int width, float rho, float theta, int threshold,
                                    int lines_max, float min_theta, float max_theta, int min_length, int max_gap,
                                    int exclusive, int options, float *lines, int *votes, unsigned int *bases,
                                    int *line_counts, int *segments, int segments_max, int *seg_counts, int *fits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !fits || !seg_counts || lines_max < 1) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    {
        const SegArgs a{min_length, max_gap, exclusive, segments_max};
        HoughGeom hg;
        int lds_rows = 0, probe = 0;
        const HoughOut out{nullptr, nullptr, nullptr, &probe, nullptr};
        if ((rc = hough_prepare(ctx, height, width, rho, theta, lines_max, min_theta, max_theta, out, hg, &lds_rows)) ||
            (rc = segments_check(height, width, n_frames, lines_max, a, true)) ||
            (rc = line_fits_check(height, width, n_frames, rho, segments_max, options, (const int *)16)))
            return rc;
    }
    const size_t slots = (size_t)n_frames * lines_max, seg_slots = (size_t)n_frames * segments_max;
    // staging: lines (2 floats per slot) | votes | bases | line counts | segment counts; the fits, then the segment records
    HIP_TRY(ctx, ctx->io[1].ensure(slots * 16 + 2 * (size_t)n_frames * sizeof(int)));
    HIP_TRY(ctx, ctx->io[2].ensure(seg_slots * (CANNY_HIP_LINE_FIT_INTS + CANNY_HIP_SEGMENT_INTS) * sizeof(int)));
    char *d = (char *)ctx->io[1].p;
    float *d_lines = (float *)d;
    int *d_votes = (int *)(d + slots * 8);
    unsigned *d_bases = (unsigned *)(d + slots * 12);
    int *d_line_counts = (int *)(d + slots * 16), *d_seg_counts = d_line_counts + n_frames;
    int *d_fits = (int *)ctx->io[2].p, *d_segments = d_fits + seg_slots * CANNY_HIP_LINE_FIT_INTS;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_hough_line_fits(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height,
                                                  width, n_frames, nullptr, rho, theta, threshold, lines_max, min_theta,
                                                  max_theta, lines ? d_lines : nullptr, votes ? d_votes : nullptr, d_bases,
                                                  d_line_counts, nullptr, min_length, max_gap, exclusive, d_segments,
                                                  segments_max, d_seg_counts, options, d_fits)))
        return rc;
    std::vector<int> cnt(2 * (size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_line_counts, cnt.size() * sizeof(int)))) return rc;
    // the counts first, then only the filled slots of each frame
    for (int f = 0; f < n_frames; f++) {
        const size_t k = (size_t)std::min(cnt[f], lines_max), at = (size_t)f * lines_max;
        if (k && lines)
            HIP_TRY(ctx, hipMemcpyAsync(lines + 2 * at, d_lines + 2 * at, k * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (k && votes) HIP_TRY(ctx, hipMemcpyAsync(votes + at, d_votes + at, k * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (k && bases) HIP_TRY(ctx, hipMemcpyAsync(bases + at, d_bases + at, k * 4, hipMemcpyDeviceToHost, ctx->stream));
        const size_t j = (size_t)std::min(cnt[(size_t)n_frames + f], segments_max);
        const size_t sat = (size_t)f * segments_max * CANNY_HIP_SEGMENT_INTS;
        const size_t fat = (size_t)f * segments_max * CANNY_HIP_LINE_FIT_INTS;
        if (j && segments)
            HIP_TRY(ctx, hipMemcpyAsync(segments + sat, d_segments + sat, j * CANNY_HIP_SEGMENT_INTS * sizeof(int),
                                        hipMemcpyDeviceToHost, ctx->stream));
        if (j)
            HIP_TRY(ctx, hipMemcpyAsync(fits + fat, d_fits + fat, j * CANNY_HIP_LINE_FIT_INTS * sizeof(int),
                                        hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (line_counts) std::memcpy(line_counts, cnt.data(), (size_t)n_frames * sizeof(int));
    std::memcpy(seg_counts, cnt.data() + n_frames, (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

int canny_hip_dev_line_fits_arith(canny_hip_ctx *ctx, const long long *d_moments, size_t n_sets, int *d_out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!n_sets || !d_moments || !d_out) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, launch_line_fits_arith(d_moments, n_sets, d_out, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_line_fits_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfLineFits, CANNY_HIP_LINE_FIT_PARTS, part, total_ms, launches);
}

int canny_hip_hough_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfHough, 3, part, total_ms, launches);
}

int canny_hip_components_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfComponents, CANNY_HIP_CC_PARTS, part, total_ms, launches);
}

int canny_hip_edt_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfEdt, CANNY_HIP_EDT_PARTS, part, total_ms, launches);
}

int canny_hip_hough_segments_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfSegments, CANNY_HIP_SEGMENT_PARTS, part, total_ms, launches);
}

int canny_hip_contours_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfContours, CANNY_HIP_CONTOUR_PARTS, part, total_ms, launches);
}

int canny_hip_polygons_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfPolygons, CANNY_HIP_POLYGON_PARTS, part, total_ms, launches);
}

// ---- Hough circles ----------------------------------------------------------------------------------------
int canny_hip_hough_circles_step_of(int gx, int gy, int *sx, int *sy)
{
    if (!sx || !sy || gx < -32768 || gx > 32767 || gy < -32768 || gy > 32767) return CANNY_HIP_ERR_INVALID;
    circles_step_of(gx, gy, sx, sy);
    return CANNY_HIP_OK;
}

int canny_hip_hough_circles_from_bits(const unsigned char *bits, const short *gx, const short *gy, int height, int width,
                                      int min_radius, int max_radius, int cell_shift, int threshold, int support_threshold,
                                      int min_dist, int centres_max, int *circles, int *count, int *centre_count,
                                      int *accum)
{
    const CircleArgs a{min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max};
    CircleGeom cg;
    if (!bits || !gx || !gy) return CANNY_HIP_ERR_INVALID;
    int rc = circles_prepare(height, width, a, count, cg);
    if (rc) return rc;
    if ((rc = check_dims(height, width, 1))) return rc;
    const int c = 1 << cell_shift, stride = cg.aw + 2, row_bytes = (width + 7) / 8;
    std::vector<int> acc((size_t)(cg.ah + 2) * stride, 0);
    std::vector<int> px, py; // the set pixels, in raster order
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            if (!(bits[(size_t)y * row_bytes + (x >> 3)] >> (7 - (x & 7)) & 1)) continue;
            px.push_back(x);
            py.push_back(y);
            int sx, sy;
            circles_step_of(gx[(size_t)y * width + x], gy[(size_t)y * width + x], &sx, &sy);
            if (!sx && !sy) continue;
            for (int s = 1; s >= -1; s -= 2)
                for (int k = min_radius; k <= max_radius; k++) {
                    const long long X = (long long)x * 1024 + (long long)s * k * sx, Y = (long long)y * 1024 + (long long)s * k * sy;
                    const long long qx = X >> 10, qy = Y >> 10;
                    if (qx < 0 || qx >= width || qy < 0 || qy >= height) break; // the frame is convex
                    acc[(size_t)((qy >> cell_shift) + 1) * stride + (qx >> cell_shift) + 1] += 1;
                }
        }
    std::vector<std::pair<int, unsigned>> peaks; // (-votes, base): ascending = votes descending, base ascending
    for (int ay = 0; ay < cg.ah; ay++)
        for (int ax = 0; ax < cg.aw; ax++) {
            const size_t b = (size_t)(ay + 1) * stride + ax + 1;
            const int v = acc[b];
            if (v > threshold && v > acc[b - 1] && v >= acc[b + 1] && v > acc[b - stride] && v >= acc[b + stride])
                peaks.emplace_back(-v, (unsigned)b);
        }
    std::sort(peaks.begin(), peaks.end());
    const int K = (int)std::min<size_t>((size_t)centres_max, peaks.size());
    const int nr = max_radius - min_radius + 1;
    std::vector<long long> hist((size_t)nr);
    std::vector<int> ax2, ay2; // accepted centres
    int n_acc = 0;
    const unsigned long long md = 2ull * (unsigned long long)min_dist;
    for (int k = 0; k < K; k++) {
        const unsigned base = peaks[k].second;
        const long long x2 = (2ll * ((int)(base % (unsigned)stride) - 1) + 1) * c;
        const long long y2 = (2ll * ((int)(base / (unsigned)stride) - 1) + 1) * c;
        std::fill(hist.begin(), hist.end(), 0);
        for (size_t i = 0; i < px.size(); i++) {
            const long long dx = 2ll * px[i] - x2, dy = 2ll * py[i] - y2, d = dx * dx + dy * dy;
            long long s = (long long)std::sqrt((double)d); // floor of the root, corrected
            while (s * s > d) s--;
            while ((s + 1) * (s + 1) <= d) s++;
            const long long r = (s + 1) >> 1; // (2r - 1)^2 <= d < (2r + 1)^2
            if (r >= min_radius && r <= max_radius) hist[(size_t)(r - min_radius)]++;
        }
        int best = min_radius;
        for (int r = min_radius + 1; r <= max_radius; r++) // count[r] / r > count[best] / best; products below 2^41
            if (hist[(size_t)(r - min_radius)] * best > hist[(size_t)(best - min_radius)] * r) best = r;
        const long long support = hist[(size_t)(best - min_radius)];
        if (support <= support_threshold) continue;
        bool near = false;
        for (size_t j = 0; j < ax2.size() && !near; j++) {
            const long long dx = x2 - ax2[j], dy = y2 - ay2[j];
            near = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy) < md * md;
        }
        if (near) continue;
        ax2.push_back((int)x2);
        ay2.push_back((int)y2);
        if (circles) {
            int *rec = circles + (size_t)n_acc * kCircleRecord;
            rec[0] = (int)x2, rec[1] = (int)y2, rec[2] = best, rec[3] = -peaks[k].first, rec[4] = (int)support;
            rec[5] = (int)base;
        }
        n_acc++;
    }
    if (accum) std::memcpy(accum, acc.data(), acc.size() * sizeof(int));
    if (centre_count) *centre_count = (int)std::min<size_t>(peaks.size(), 0x7fffffff);
    *count = n_acc;
    return CANNY_HIP_OK;
}

int canny_hip_dev_hough_circles_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, const short *d_gx, const short *d_gy,
                                     int n_frames, int height, int width, int min_radius, int max_radius, int cell_shift,
                                     int threshold, int support_threshold, int min_dist, int centres_max, int *d_circles,
                                     int *d_counts, int *d_centre_counts, int *d_accum)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_gx || !d_gy) return CANNY_HIP_ERR_INVALID;
    const CircleArgs a{min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max};
    CircleGeom cg;
    if ((rc = circles_prepare(height, width, a, d_counts, cg)) || (rc = check_dims(height, width, n_frames)) ||
        (rc = finish_pending(ctx)))
        return rc;
    return dev_circles(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), nullptr, false, d_gx, d_gy, cg, a,
                       CircleOut{d_circles, d_counts, d_centre_counts, d_accum});
}

int canny_hip_dev_canny_hough_circles(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                      int height, int width, int n_frames, short *d_edges, int min_radius, int max_radius,
                                      int cell_shift, int threshold, int support_threshold, int min_dist, int centres_max,
                                      int *d_circles, int *d_counts, int *d_centre_counts, int *d_accum)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img) return CANNY_HIP_ERR_INVALID;
    const CircleArgs a{min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max};
    CircleGeom cg;
    if ((rc = circles_prepare(height, width, a, d_counts, cg)) || (rc = check_dims(height, width, n_frames))) return rc;
    const uint64_t *strong;
    if ((rc = dev_canny_map(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, &strong))) return rc;
    // every route of dev_canny leaves the whole batch's smoothed plane in ctx->smoothed, as bytes iff last_canny_u8
    // 
    return dev_circles(ctx, strong, nullptr, make_hyst_geom(height, width, n_frames), ctx->smoothed.p,
                       ctx->last_canny_u8 != 0, nullptr, nullptr, cg, a,
                       CircleOut{d_circles, d_counts, d_centre_counts, d_accum});
}

int canny_hip_canny_hough_circles(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                  int max_val, int height, int width, int min_radius, int max_radius, int cell_shift,
                                  int threshold, int support_threshold, int min_dist, int centres_max, int *circles,
                                  int *counts, int *centre_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs) return CANNY_HIP_ERR_INVALID;
    {
        const CircleArgs a{min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max};
        CircleGeom cg;
        if ((rc = circles_prepare(height, width, a, counts, cg)) || (rc = check_dims(height, width, n_frames))) return rc;
    }
    const size_t slots = (size_t)n_frames * centres_max;
    // one staging block: records (6 ints per slot) | counts | centre counts
    HIP_TRY(ctx, ctx->io[1].ensure((slots * kCircleRecord + 2 * (size_t)n_frames) * sizeof(int)));
    int *d_rec = (int *)ctx->io[1].p, *d_cnt = d_rec + slots * kCircleRecord;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_hough_circles(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height,
                                                width, n_frames, nullptr, min_radius, max_radius, cell_shift, threshold,
                                                support_threshold, min_dist, centres_max, circles ? d_rec : nullptr, d_cnt,
                                                d_cnt + n_frames, nullptr)))
        return rc;
    std::vector<int> cnt(2 * (size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_cnt, cnt.size() * sizeof(int)))) return rc;
    // only the circles come down: the filled slots of each frame
    for (int f = 0; circles && f < n_frames; f++) {
        const size_t k = (size_t)cnt[f], at = (size_t)f * centres_max * kCircleRecord;
        if (k) HIP_TRY(ctx, hipMemcpyAsync(circles + at, d_rec + at, k * kCircleRecord * sizeof(int), hipMemcpyDeviceToHost,
                                          ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(counts, cnt.data(), (size_t)n_frames * sizeof(int));
    if (centre_counts) std::memcpy(centre_counts, cnt.data() + n_frames, (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

int canny_hip_dev_hough_circles_steps(canny_hip_ctx *ctx, const short *d_gx, const short *d_gy, size_t n, int *d_sx,
                                      int *d_sy)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_gx || !d_gy || !d_sx || !d_sy || !n) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, launch_circles_steps(d_gx, d_gy, n, d_sx, d_sy, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_hough_circles_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfCircles, CANNY_HIP_CIRCLE_PARTS, part, total_ms, launches);
}

// ---- sub-pixel circle fits (canny_circle_fits.hip) --------------------------------
namespace {

// THE check of the fit arguments; needs no device and writes nothing
int circle_fits_check(int height, int width, int n_frames, int centres_max, int band, int trim_q8, int options,
                      const int *d_fits)
{
    if ((options & ~(CANNY_HIP_CIRCLE_FIT_GATE | CANNY_HIP_CIRCLE_FIT_REFINED_ONLY)) || !d_fits || ((uintptr_t)d_fits & 15) ||
        centres_max < 1 || band < 0 || trim_q8 < 0 || height < 2 || width < 2)
        return CANNY_HIP_ERR_INVALID;
    if (std::max(height, width) > CANNY_HIP_CIRCLE_FIT_MAX_AXIS || band > CANNY_HIP_CIRCLE_FIT_MAX_BAND)
        return CANNY_HIP_ERR_UNSUPPORTED;
    if ((double)n_frames * (double)centres_max * CANNY_HIP_CIRCLE_FIT_INTS >= 2147483648.0) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// the fits of the circle records in d_circles, queued on the context's stream
int dev_circle_fits(canny_hip_ctx *ctx, const uint64_t *strong, const uint8_t *bits, const HystGeom &g, const int *d_circles,
                    const int *d_counts, int centres_max, const void *d_plane, bool plane_u8, int band, int trim_q8,
                    int options, int *d_fits)
{
    StageTimer tm(ctx, canny_hip_ctx::kProfCircleFits + CANNY_HIP_CIRCLE_FIT_PART_FIT);
    HIP_TRY(ctx, launch_circle_fits(strong, bits, g, d_circles, d_counts, centres_max, d_plane, plane_u8, band, trim_q8,
                                    options, d_fits, ctx->stream));
    return CANNY_HIP_OK;
}

} // namespace

int canny_hip_circle_fits_queue_capacity(void) { return circle_fits_queue_capacity(); }

int canny_hip_dev_circle_fits_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, const void *d_plane, int plane_is_u8,
                                   int n_frames, int height, int width, const int *d_circles, const int *d_counts,
                                   int centres_max, int band, int trim_q8, int options, int *d_fits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_circles || !d_counts) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    if ((rc = circle_fits_check(height, width, n_frames, centres_max, band, trim_q8, options, d_fits))) return rc;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, height, width) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        d_plane = ctx->smoothed.p;
        plane_is_u8 = ctx->last_canny_u8;
    }
    if ((rc = finish_pending(ctx))) return rc;
    return dev_circle_fits(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), d_circles, d_counts, centres_max,
                           d_plane, plane_is_u8 != 0, band, trim_q8, options, d_fits);
}

int canny_hip_dev_canny_hough_circle_fits(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                          int max_val, int height, int width, int n_frames, short *d_edges, int min_radius,
                                          int max_radius, int cell_shift, int threshold, int support_threshold,
                                          int min_dist, int centres_max, int *d_circles, int *d_counts,
                                          int *d_centre_counts, int *d_accum, int band, int trim_q8, int options,
                                          int *d_fits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img) return CANNY_HIP_ERR_INVALID;
    {
        const CircleArgs a{min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max};
        CircleGeom cg;
        int probe = 0;
        if ((rc = circles_prepare(height, width, a, &probe, cg)) || (rc = check_dims(height, width, n_frames)) ||
            (rc = circle_fits_check(height, width, n_frames, centres_max, band, trim_q8, options, d_fits)))
            return rc;
    }
    // the fits need the records and the counts: the context's own where the caller wants none
    const size_t slots = (size_t)n_frames * centres_max;
    if (!d_circles || !d_counts) {
        HIP_TRY(ctx, ctx->circ_recs.ensure((slots * kCircleRecord + (size_t)n_frames) * sizeof(int)));
        int *own = (int *)ctx->circ_recs.p;
        if (!d_circles) d_circles = own;
        if (!d_counts) d_counts = own + slots * kCircleRecord;
    }
    if ((rc = canny_hip_dev_canny_hough_circles(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges,
                                                min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist,
                                                centres_max, d_circles, d_counts, d_centre_counts, d_accum)))
        return rc;
    if (max_val > 255) return CANNY_HIP_OK; // the empty map: every count is 0
    return dev_circle_fits(ctx, (const uint64_t *)ctx->plane_s.p, nullptr, make_hyst_geom(height, width, n_frames), d_circles,
                           d_counts, centres_max, ctx->smoothed.p, ctx->last_canny_u8 != 0, band, trim_q8, options, d_fits);
}

int canny_hip_canny_hough_circle_fits(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                      int max_val, int height, int width, int min_radius, int max_radius, int cell_shift,
                                      int threshold, int support_threshold, int min_dist, int centres_max, int band,
                                      int trim_q8, int options, int *circles, int *counts, int *centre_counts, int *fits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !fits) return CANNY_HIP_ERR_INVALID;
    {
        const CircleArgs a{min_radius, max_radius, cell_shift, threshold, support_threshold, min_dist, centres_max};
        CircleGeom cg;
        if ((rc = circles_prepare(height, width, a, counts, cg)) || (rc = check_dims(height, width, n_frames)) ||
            (rc = circle_fits_check(height, width, n_frames, centres_max, band, trim_q8, options, (const int *)16)))
            return rc;
    }
    const size_t slots = (size_t)n_frames * centres_max;
    // staging: fits (8 ints per slot, 16-byte aligned at the block's start) | records (6 ints per slot) | counts | centre counts
    HIP_TRY(ctx, ctx->io[1].ensure((slots * (CANNY_HIP_CIRCLE_FIT_INTS + kCircleRecord) + 2 * (size_t)n_frames) * sizeof(int)));
    int *d_fits = (int *)ctx->io[1].p, *d_rec = d_fits + slots * CANNY_HIP_CIRCLE_FIT_INTS;
    int *d_cnt = d_rec + slots * kCircleRecord;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_hough_circle_fits(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height,
                                                    width, n_frames, nullptr, min_radius, max_radius, cell_shift, threshold,
                                                    support_threshold, min_dist, centres_max, d_rec, d_cnt, d_cnt + n_frames,
                                                    nullptr, band, trim_q8, options, d_fits)))
        return rc;
    std::vector<int> cnt(2 * (size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_cnt, cnt.size() * sizeof(int)))) return rc;
    // the counts first, then only the filled slots of each frame
    for (int f = 0; f < n_frames; f++) {
        const size_t k = (size_t)cnt[f], at = (size_t)f * centres_max;
        if (k && circles)
            HIP_TRY(ctx, hipMemcpyAsync(circles + at * kCircleRecord, d_rec + at * kCircleRecord,
                                        k * kCircleRecord * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (k)
            HIP_TRY(ctx, hipMemcpyAsync(fits + at * CANNY_HIP_CIRCLE_FIT_INTS, d_fits + at * CANNY_HIP_CIRCLE_FIT_INTS,
                                        k * CANNY_HIP_CIRCLE_FIT_INTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(counts, cnt.data(), (size_t)n_frames * sizeof(int));
    if (centre_counts) std::memcpy(centre_counts, cnt.data() + n_frames, (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

int canny_hip_dev_circle_fits_arith(canny_hip_ctx *ctx, const long long *d_moments, size_t n_sets, int *d_out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!n_sets || !d_moments || !d_out) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, launch_circle_fits_arith(d_moments, n_sets, d_out, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_circle_fits_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfCircleFits, CANNY_HIP_CIRCLE_FIT_PARTS, part, total_ms, launches);
}

// ---- measurement aid ------------------------------------------------------------------------------------
int canny_hip_probe_copy(canny_hip_ctx *ctx, const void *d_src, void *d_dst, size_t nbytes, int launches,
                         double *avg_ms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_src || !d_dst || !avg_ms || launches < 1 || launches > 10000 || nbytes < 16 || (nbytes & 15) ||
        ((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 15))
        return CANNY_HIP_ERR_INVALID;
    hipEvent_t a = nullptr, b = nullptr;
    HIP_TRY(ctx, hipEventCreate(&a));
    {
        const hipError_t eb = hipEventCreate(&b);
        if (eb != hipSuccess) {
            (void)hipEventDestroy(a);
            return fail(ctx, eb, "hipEventCreate");
        }
    }
    double total = 0.0;
    hipError_t e = hipSuccess;
    for (int k = 0; k < launches && e == hipSuccess; k++) {
        // the event pair is attached to the dispatch: the kernel's own begin / end timestamps
        e = launch_probe_copy(d_src, d_dst, nbytes, ctx->stream, LaunchEvents{a, b});
        if (e == hipSuccess) e = hipEventSynchronize(b);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
        total += ms;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    HIP_TRY(ctx, e);
    *avg_ms = total / launches;
    return CANNY_HIP_OK;
}

// Host-only: the cell order of the marching launches (march_cell_of), for the bijectivity test.
int canny_hip_selftest_march_order(int n_segs, int n_strips, int *out_pairs)
{
    if (!out_pairs || n_segs < 1 || n_strips < 1 || (long long)n_segs * n_strips > (1 << 24)) return CANNY_HIP_ERR_INVALID;
    for (int k = 0; k < n_segs * n_strips; k++) {
        const MarchCell c = march_cell_of(k, n_segs, n_strips);
        out_pairs[2 * k] = c.seg;
        out_pairs[2 * k + 1] = c.strip;
    }
    return CANNY_HIP_OK;
}

// Host-only: the launch plan of a capped grid, from the helper its launchers take their grid from (canny_kernels.h).
int canny_hip_selftest_launch_plan(int kind, int n_frames, int height, int width, long long extra,
                                   unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    LaunchPlan p;
    switch (kind) {
    case CANNY_HIP_PLAN_CC_FIXUP:
    case CANNY_HIP_PLAN_PG_RECORDS:
    case CANNY_HIP_PLAN_PG_SCAN_SUMS:
    case CANNY_HIP_PLAN_HOUGH_CELLS:
    case CANNY_HIP_PLAN_CIRCLES_STEPS:
    case CANNY_HIP_PLAN_TO_GRAY: // sized by `extra` alone
        if (extra < 1) return CANNY_HIP_ERR_INVALID;
        p = kind == CANNY_HIP_PLAN_CC_FIXUP       ? plan_cc_fixup((unsigned long long)extra)
            : kind == CANNY_HIP_PLAN_PG_RECORDS   ? plan_pg_records((unsigned long long)extra)
            : kind == CANNY_HIP_PLAN_PG_SCAN_SUMS ? plan_pg_scan_sums((unsigned long long)extra)
            : kind == CANNY_HIP_PLAN_HOUGH_CELLS  ? plan_hough_cells((unsigned long long)extra)
            : kind == CANNY_HIP_PLAN_CIRCLES_STEPS ? plan_circles_steps((size_t)extra)
                                                  : plan_to_gray((size_t)extra);
        break;
    case CANNY_HIP_PLAN_SCAN_FRAMES:
        if (check_dims(1, 1, n_frames)) return CANNY_HIP_ERR_INVALID;
        p = plan_scan_frames(n_frames);
        break;
    default: {
        if (kind < 0 || kind >= CANNY_HIP_PLAN_KINDS || check_dims(height, width, n_frames))
            return CANNY_HIP_ERR_INVALID;
        const HystGeom g = make_hyst_geom(height, width, n_frames);
        switch (kind) {
        case CANNY_HIP_PLAN_POINTS_ROWS: p = plan_points_rows(g); break;
        case CANNY_HIP_PLAN_CC_TILES: p = plan_cc_tiles(g); break;
        case CANNY_HIP_PLAN_CC_ROWS: p = plan_cc_rows(g); break;
        case CANNY_HIP_PLAN_CT_ROWS: p = plan_ct_rows(g); break;
        case CANNY_HIP_PLAN_EDT_ROWS: p = plan_edt_rows(g); break;
        case CANNY_HIP_PLAN_EDT_COLUMNS: p = plan_edt_columns(g); break;
        case CANNY_HIP_PLAN_HOUGH_VOTE_STRONG: p = plan_hough_vote_global(g, kSrcStrong); break;
        case CANNY_HIP_PLAN_HOUGH_VOTE_BITS: p = plan_hough_vote_global(g, kSrcBits); break;
        case CANNY_HIP_PLAN_HOUGH_VOTE_POINTS: // the frame's points are the caller's to say
            if (extra < 0) return CANNY_HIP_ERR_INVALID;
            p = plan_hough_vote_global(g, kSrcPoints, (unsigned long long)extra);
            break;
        case CANNY_HIP_PLAN_CIRCLES_VOTE_STRONG: p = plan_circles_vote(g, false); break;
        case CANNY_HIP_PLAN_CIRCLES_VOTE_BITS: p = plan_circles_vote(g, true); break;
        default: return CANNY_HIP_ERR_INVALID;
        }
    }
    }
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// Host-only: the batch pipelines' bit-map expansion (ExpandPool) on a caller-supplied bit map; needs no device.
int canny_hip_selftest_expand_bits(const unsigned char *bits, int height, int width, int to_u8, void *out, int n_threads)
{
    if (!bits || !out || height < 1 || width < 1 || n_threads < 1 || n_threads > 64) return CANNY_HIP_ERR_INVALID;
    ExpandPool pool(n_threads);
    constexpr int kBlockRows = 128;
    const int row_bytes = (width + 7) / 8, blocks = (height + kBlockRows - 1) / kBlockRows;
    std::atomic<int> left{blocks};
    for (int b = 0; b < blocks; b++) {
        ExpandPool::Job job;
        const int r0 = b * kBlockRows;
        job.bits = bits + (size_t)r0 * row_bytes;
        job.dst = (unsigned char *)out + (size_t)r0 * width * (to_u8 ? 1 : sizeof(short));
        job.rows = std::min(kBlockRows, height - r0);
        job.width = width;
        job.row_bytes = row_bytes;
        job.to_u8 = to_u8 != 0;
        job.left = &left;
        pool.submit(job);
    }
    pool.wait(left);
    return CANNY_HIP_OK;
}

// ---- self-test ----------------------------------------------------------------------------------------
int canny_hip_selftest_mag_angle(canny_hip_ctx *ctx, int lim, short *magnitudes, unsigned char *bins)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!magnitudes || !bins || lim < 0 || lim > 1020) return CANNY_HIP_ERR_INVALID;
    size_t total = (size_t)(2 * lim + 1) * (2 * lim + 1);
    HIP_TRY(ctx, ctx->io[0].ensure(total * 2));
    HIP_TRY(ctx, ctx->io[1].ensure(total));
    HIP_TRY(ctx, launch_selftest_mag_angle(lim, (int16_t *)ctx->io[0].p, (uint8_t *)ctx->io[1].p, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(magnitudes, ctx->io[0].p, total * 2, hipMemcpyDeviceToHost, ctx->stream));
    return d2h_sync(ctx, bins, ctx->io[1].p, total);
}

int canny_hip_selftest_sobel_pixel(canny_hip_ctx *ctx, int form, int lim, short *magnitudes, unsigned char *bins)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!magnitudes || !bins || lim < 0 || lim > 1020 || form < CANNY_HIP_PIXEL_LDS_TILE ||
        form > CANNY_HIP_PIXEL_F32_FLOOR)
        return CANNY_HIP_ERR_INVALID;
    size_t total = (size_t)(2 * lim + 1) * (2 * lim + 1);
    HIP_TRY(ctx, ctx->io[0].ensure(total * 2));
    HIP_TRY(ctx, ctx->io[1].ensure(total));
    int16_t *d_mags = (int16_t *)ctx->io[0].p;
    uint8_t *d_bins = (uint8_t *)ctx->io[1].p;
    if (form == CANNY_HIP_PIXEL_LDS_TILE)
        HIP_TRY(ctx, launch_selftest_mag_angle(lim, d_mags, d_bins, ctx->stream));
    else
        HIP_TRY(ctx, launch_selftest_sobel_pixel(form, lim, d_mags, d_bins, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(magnitudes, d_mags, total * 2, hipMemcpyDeviceToHost, ctx->stream));
    return d2h_sync(ctx, bins, d_bins, total);
}

static int selftest_div_common(canny_hip_ctx *ctx, float divisor, int use_fma, float c,
                               unsigned long long *mismatches, float *largest_mismatching_dividend)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!mismatches || !largest_mismatching_dividend || !(divisor > 0.0f) || !std::isfinite(divisor))
        return CANNY_HIP_ERR_INVALID;
    HIP_TRY(ctx, ctx->io[0].ensure(2 * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->io[0].p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    const unsigned last = 0x43800000u; // bit pattern of 256.0f; non-negative floats are ordered like their bits
    HIP_TRY(ctx, launch_selftest_div(divisor, use_fma, c, 0u, last, (unsigned long long *)ctx->io[0].p, ctx->stream));
    unsigned long long res[2] = {0, 0};
    if ((rc = d2h_sync(ctx, res, ctx->io[0].p, sizeof(res)))) return rc;
    *mismatches = res[0];
    unsigned bits = (unsigned)res[1];
    std::memcpy(largest_mismatching_dividend, &bits, sizeof(float));
    return CANNY_HIP_OK;
}

int canny_hip_selftest_div(canny_hip_ctx *ctx, float divisor, unsigned long long *mismatches,
                           float *largest_mismatching_dividend)
{
    return selftest_div_common(ctx, divisor, 0, 0.0f, mismatches, largest_mismatching_dividend);
}

int canny_hip_selftest_div_fma_table(int index, float *divisor, float *c)
{
    const unsigned(*table)[2] = nullptr;
    const int n = gaussian_fma_div_table(&table);
    if (index < 0 || index >= n || !divisor || !c) return CANNY_HIP_ERR_INVALID;
    std::memcpy(divisor, &table[index][0], sizeof(float));
    std::memcpy(c, &table[index][1], sizeof(float));
    return CANNY_HIP_OK;
}

int canny_hip_selftest_div_fma(canny_hip_ctx *ctx, float divisor, float c, unsigned long long *mismatches,
                               float *largest_mismatching_dividend)
{
    return selftest_div_common(ctx, divisor, 1, c, mismatches, largest_mismatching_dividend);
}

// The histogram and select passes of the automatic rules on their own, launched as dev_canny launches them.
int canny_hip_selftest_histogram(canny_hip_ctx *ctx, const void *d_plane, int plane_is_u8, int kind, int height, int width,
                                 int n_frames, unsigned int *d_hist)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_plane || !d_hist || (kind != kAutoMedian && kind != kAutoQuantile)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)n_frames * kHistBins * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, kind == kAutoMedian
                     ? launch_hist_intensity(d_plane, plane_is_u8 != 0, d_hist, height, width, n_frames, ctx->stream)
                     : launch_hist_gradient(d_plane, plane_is_u8 != 0, d_hist, height, width, n_frames, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_selftest_select(canny_hip_ctx *ctx, const unsigned int *d_hist, int n_frames, int rule, float low, float high,
                              int *d_pairs)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_hist || !d_pairs || !auto_params_valid(rule, low, high)) return CANNY_HIP_ERR_INVALID;
    if ((rc = check_dims(1, 1, n_frames))) return rc;
    HIP_TRY(ctx, launch_thr_select(d_hist, n_frames, rule, low, high, d_pairs, ctx->stream));
    return CANNY_HIP_OK;
}

// Workspace `index` of the context as it stands: no launch, no allocation, nothing of the workspaces changes.
int canny_hip_selftest_workspace(canny_hip_ctx *ctx, int index, const char **name, void **d_ptr, size_t *bytes, int *kind)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (index < 0 || !name || !d_ptr || !bytes || !kind) return CANNY_HIP_ERR_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->has_pend) return CANNY_HIP_ERR_INVALID; // a streamed batch's sweeps still own the planes
    std::vector<WsEntry> all;
    collect_workspaces(ctx, "", all);
    if ((size_t)index >= all.size()) return CANNY_HIP_ERR_INVALID;
    ctx->ws_name = all[(size_t)index].name;
    *name = ctx->ws_name.c_str();
    *d_ptr = all[(size_t)index].buf->p;
    *bytes = all[(size_t)index].buf->bytes;
    *kind = all[(size_t)index].kind;
    return CANNY_HIP_OK;
}

// ---- chamfer template matching (canny_chamfer.hip) ---------------------------------
} // extern "C"

struct canny_hip_chamfer_set {
    canny_hip_ctx *ctx = nullptr;
    ChamferLayout lay;
    DevBuf dev; // offsets | points | boxes | band offsets | bands
    ChamferSetDev d{};
};

namespace {

struct ChamferArgs {
    int trunc_q4, max_mean_q4, min_dist, matches_max;
};
struct ChamferOut {
    int *d_matches, *d_counts, *d_cand_counts;
    unsigned *d_scores;
};

// Whether `set` is a live set of this context.  The handle is looked up among the sets the context created and has not
// destroyed, and is not read: a destroyed set's memory is gone, a foreign one belongs to another context's list.
bool chamfer_set_alive(const canny_hip_ctx *ctx, const canny_hip_chamfer_set *set)
{
    return set && std::find(ctx->chamfer_sets.begin(), ctx->chamfer_sets.end(), set) != ctx->chamfer_sets.end();
}

// THE check of the matching arguments; needs no device and writes nothing
int chamfer_check(const canny_hip_ctx *ctx, int height, int width, int n_frames, const canny_hip_chamfer_set *set,
                  const ChamferArgs &a, const int *d_counts)
{
    if (!chamfer_set_alive(ctx, set) || !d_counts || a.trunc_q4 < 1 || a.max_mean_q4 < 0 || a.max_mean_q4 >= a.trunc_q4 ||
        a.min_dist < 0 || a.matches_max < 1)
        return CANNY_HIP_ERR_INVALID;
    int rc = check_dims(height, width, n_frames);
    if (rc) return rc;
    if (a.trunc_q4 > CANNY_HIP_CHAMFER_MAX_TRUNC || a.matches_max > kHoughMaxLines || height > 65535 || width > 65535 ||
        (long long)height * width * set->lay.n_templates >= 0x80000000LL)
        return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// The matching of n frames of a device dist2 plane, queued on the context's stream, chunk of frames by chunk of frames.
int dev_chamfer(canny_hip_ctx *ctx, const int *d_dist2, int n, int h, int w, const canny_hip_chamfer_set *set,
                const ChamferArgs &a, const ChamferOut &out)
{
    const int T = set->lay.n_templates;
    const size_t hw = (size_t)h * w;
    const int chunk = chamfer_chunk_frames(n, h, w, T, out.d_scores != nullptr, ctx->chamfer_chunk_mb);
    const bool tiled = (ctx->chamfer_route ? ctx->chamfer_route : chamfer_auto_route(set->lay)) == 2;
    HIP_TRY(ctx, ctx->chamfer_cost.ensure((size_t)chunk * hw * sizeof(uint16_t)));
    if (!out.d_scores) HIP_TRY(ctx, ctx->chamfer_scores.ensure((size_t)chunk * hw * T * sizeof(unsigned)));
    HIP_TRY(ctx, ctx->chamfer_ws.ensure(chamfer_ws_bytes(chunk, a.matches_max)));
    uint16_t *cost = (uint16_t *)ctx->chamfer_cost.p;
    const int part = canny_hip_ctx::kProfChamfer;
    for (int f0 = 0; f0 < n; f0 += chunk) {
        const int nf = std::min(chunk, n - f0);
        unsigned *scores = out.d_scores ? out.d_scores + (size_t)f0 * hw * T : (unsigned *)ctx->chamfer_scores.p;
        {
            StageTimer tm(ctx, part + CANNY_HIP_CHAMFER_PART_COST);
            HIP_TRY(ctx, launch_chamfer_cost(d_dist2 + (size_t)f0 * hw, (size_t)nf * hw, a.trunc_q4, cost, ctx->stream));
        }
        {
            StageTimer tm(ctx, part + CANNY_HIP_CHAMFER_PART_SCORE);
            HIP_TRY(ctx, launch_chamfer_score(cost, nf, h, w, set->d, a.trunc_q4, tiled, scores, ctx->stream));
        }
        {
            StageTimer tm(ctx, part + CANNY_HIP_CHAMFER_PART_CANDIDATES);
            HIP_TRY(ctx, launch_chamfer_candidates(scores, nf, h, w, set->d, a.max_mean_q4, a.matches_max, ctx->chamfer_ws.p,
                                                   out.d_cand_counts ? out.d_cand_counts + f0 : nullptr, ctx->stream));
        }
        {
            StageTimer tm(ctx, part + CANNY_HIP_CHAMFER_PART_ACCEPT);
            HIP_TRY(ctx, launch_chamfer_accept(scores, nf, h, w, T, a.matches_max, a.min_dist, ctx->chamfer_ws.p,
                                               out.d_matches ? out.d_matches + (size_t)f0 * a.matches_max * CANNY_HIP_MATCH_INTS
                                                             : nullptr,
                                               out.d_counts + f0, ctx->stream));
        }
    }
    return CANNY_HIP_OK;
}

} // namespace

extern "C" {

int canny_hip_chamfer_set_create(canny_hip_ctx *ctx, const int *offsets, const short *points, int n_templates,
                                 canny_hip_chamfer_set **set)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!set) return CANNY_HIP_ERR_INVALID;
    *set = nullptr;
    std::unique_ptr<canny_hip_chamfer_set> s(new (std::nothrow) canny_hip_chamfer_set());
    if (!s) return CANNY_HIP_ERR_RUNTIME;
    if ((rc = chamfer_build_layout(offsets, points, n_templates, s->lay))) return rc;
    const ChamferLayout &L = s->lay;
    const size_t b_off = L.offsets.size() * sizeof(int), b_pts = L.points.size() * sizeof(uint32_t);
    const size_t b_box = L.boxes.size() * sizeof(ChamferBox), b_bo = L.band_offsets.size() * sizeof(int);
    const size_t b_bands = L.bands.size() * sizeof(ChamferBand);
    HIP_TRY(ctx, s->dev.ensure(b_off + b_pts + b_box + b_bo + b_bands));
    char *p = (char *)s->dev.p;
    s->d.offsets = (const int *)p;
    s->d.points = (const uint32_t *)(p + b_off);
    s->d.boxes = (const ChamferBox *)(p + b_off + b_pts);
    s->d.band_offsets = (const int *)(p + b_off + b_pts + b_box);
    s->d.bands = (const ChamferBand *)(p + b_off + b_pts + b_box + b_bo);
    s->d.n_templates = L.n_templates;
    s->d.max_elems = L.max_elems;
    hipError_t e = hipMemcpyAsync((void *)s->d.offsets, L.offsets.data(), b_off, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((void *)s->d.points, L.points.data(), b_pts, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((void *)s->d.boxes, L.boxes.data(), b_box, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync((void *)s->d.band_offsets, L.band_offsets.data(), b_bo, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((void *)s->d.bands, L.bands.data(), b_bands, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        s->dev.release();
        return fail(ctx, e, "canny_hip_chamfer_set_create");
    }
    s->ctx = ctx;
    ctx->chamfer_sets.push_back(s.get());
    *set = s.release();
    return CANNY_HIP_OK;
}

int canny_hip_chamfer_set_destroy(canny_hip_ctx *ctx, canny_hip_chamfer_set *set)
{
    if (!ctx || !set) return CANNY_HIP_ERR_INVALID;
    // looked up before it is read: a destroyed or foreign handle is refused without touching its memory
    auto it = std::find(ctx->chamfer_sets.begin(), ctx->chamfer_sets.end(), set);
    if (it == ctx->chamfer_sets.end()) return CANNY_HIP_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream); // a queued launch may still read the set
    ctx->chamfer_sets.erase(it);
    set->dev.release();
    delete set;
    return CANNY_HIP_OK;
}

int canny_hip_dev_chamfer_dist2(canny_hip_ctx *ctx, const int *d_dist2, int n_frames, int height, int width,
                                const canny_hip_chamfer_set *set, int trunc_q4, int max_mean_q4, int min_dist,
                                int matches_max, int *d_matches, int *d_counts, int *d_cand_counts, unsigned int *d_scores)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_dist2) return CANNY_HIP_ERR_INVALID;
    const ChamferArgs a{trunc_q4, max_mean_q4, min_dist, matches_max};
    if ((rc = chamfer_check(ctx, height, width, n_frames, set, a, d_counts)) || (rc = finish_pending(ctx))) return rc;
    return dev_chamfer(ctx, d_dist2, n_frames, height, width, set, a, ChamferOut{d_matches, d_counts, d_cand_counts, d_scores});
}

int canny_hip_dev_chamfer_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int height, int width,
                               int *d_dist2, const canny_hip_chamfer_set *set, int trunc_q4, int max_mean_q4, int min_dist,
                               int matches_max, int *d_matches, int *d_counts, int *d_cand_counts, unsigned int *d_scores)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits) return CANNY_HIP_ERR_INVALID;
    const ChamferArgs a{trunc_q4, max_mean_q4, min_dist, matches_max};
    if ((rc = chamfer_check(ctx, height, width, n_frames, set, a, d_counts)) ||
        (rc = check_edt_dims(height, width, n_frames)) || (rc = finish_pending(ctx)))
        return rc;
    if (!d_dist2) {
        HIP_TRY(ctx, ctx->chamfer_dist2.ensure(npx(height, width, n_frames) * sizeof(int)));
        d_dist2 = (int *)ctx->chamfer_dist2.p;
    }
    if ((rc = dev_edt(ctx, nullptr, d_bits, make_hyst_geom(height, width, n_frames), EdtOut{d_dist2, nullptr, nullptr})))
        return rc;
    return dev_chamfer(ctx, d_dist2, n_frames, height, width, set, a, ChamferOut{d_matches, d_counts, d_cand_counts, d_scores});
}

int canny_hip_dev_canny_chamfer(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                int height, int width, int n_frames, short *d_edges, int *d_dist2,
                                const canny_hip_chamfer_set *set, int trunc_q4, int max_mean_q4, int min_dist,
                                int matches_max, int *d_matches, int *d_counts, int *d_cand_counts, unsigned int *d_scores)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img) return CANNY_HIP_ERR_INVALID;
    const ChamferArgs a{trunc_q4, max_mean_q4, min_dist, matches_max};
    if ((rc = chamfer_check(ctx, height, width, n_frames, set, a, d_counts)) || (rc = check_edt_dims(height, width, n_frames)))
        return rc;
    if (!d_dist2) {
        HIP_TRY(ctx, ctx->chamfer_dist2.ensure(npx(height, width, n_frames) * sizeof(int)));
        d_dist2 = (int *)ctx->chamfer_dist2.p;
    }
    if ((rc = dev_canny_edt(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges,
                            EdtOut{d_dist2, nullptr, nullptr})))
        return rc;
    return dev_chamfer(ctx, d_dist2, n_frames, height, width, set, a, ChamferOut{d_matches, d_counts, d_cand_counts, d_scores});
}

int canny_hip_canny_chamfer(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                            int max_val, int height, int width, const canny_hip_chamfer_set *set, int trunc_q4,
                            int max_mean_q4, int min_dist, int matches_max, int *matches, int *counts, int *cand_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs) return CANNY_HIP_ERR_INVALID;
    const ChamferArgs a{trunc_q4, max_mean_q4, min_dist, matches_max};
    if ((rc = chamfer_check(ctx, height, width, n_frames, set, a, counts)) || (rc = check_edt_dims(height, width, n_frames)))
        return rc;
    const size_t slots = (size_t)n_frames * matches_max;
    // one staging block: records (6 ints per slot) | counts | candidate counts
    HIP_TRY(ctx, ctx->io[1].ensure((slots * CANNY_HIP_MATCH_INTS + 2 * (size_t)n_frames) * sizeof(int)));
    int *d_rec = (int *)ctx->io[1].p, *d_cnt = d_rec + slots * CANNY_HIP_MATCH_INTS;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_chamfer(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                          n_frames, nullptr, nullptr, set, trunc_q4, max_mean_q4, min_dist, matches_max,
                                          matches ? d_rec : nullptr, d_cnt, d_cnt + n_frames, nullptr)))
        return rc;
    std::vector<int> cnt(2 * (size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_cnt, cnt.size() * sizeof(int)))) return rc;
    for (int f = 0; matches && f < n_frames; f++) { // only the filled slots of each frame come down
        const size_t k = (size_t)cnt[f], at = (size_t)f * matches_max * CANNY_HIP_MATCH_INTS;
        if (k) HIP_TRY(ctx, hipMemcpyAsync(matches + at, d_rec + at, k * CANNY_HIP_MATCH_INTS * sizeof(int),
                                          hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(counts, cnt.data(), (size_t)n_frames * sizeof(int));
    if (cand_counts) std::memcpy(cand_counts, cnt.data() + n_frames, (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

// canny_hip_chamfer_from_dist2 and canny_hip_chamfer_cost_of, the rule in plain C++, live in canny_chamfer_host.cpp.

int canny_hip_dev_chamfer_costs(canny_hip_ctx *ctx, const int *d_dist2, size_t n, int trunc_q4, unsigned int *d_costs)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_dist2 || !d_costs || !n || trunc_q4 < 0) return CANNY_HIP_ERR_INVALID;
    if (trunc_q4 > CANNY_HIP_CHAMFER_MAX_TRUNC) return CANNY_HIP_ERR_UNSUPPORTED;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, launch_chamfer_costs_hook(d_dist2, n, trunc_q4, d_costs, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_chamfer_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfChamfer, CANNY_HIP_CHAMFER_PARTS, part, total_ms, launches);
}

int canny_hip_shapes_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfShapes, CANNY_HIP_SHAPE_PARTS, part, total_ms, launches);
}

int canny_hip_curves_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfCurves, CANNY_HIP_CURVE_PARTS, part, total_ms, launches);
}

// Host-only: the launch plan of the edge curves' row kernels.
int canny_hip_selftest_curves_plan(int n_frames, int height, int width, unsigned long long *out)
{
    if (!out || check_contour_dims(height, width, n_frames)) return CANNY_HIP_ERR_INVALID;
    const LaunchPlan p = plan_cv_rows(make_hyst_geom(height, width, n_frames));
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// Host-only: the launch plans of the capped launches of the contour shape measures.
int canny_hip_selftest_shapes_plan(int which, unsigned long long capacity, unsigned long long *out)
{
    if (!out || capacity < 1) return CANNY_HIP_ERR_INVALID;
    LaunchPlan p;
    if (which == CANNY_HIP_SHAPES_PLAN_RECORDS) p = plan_sh_records(capacity);
    else if (which == CANNY_HIP_SHAPES_PLAN_SCAN_SUMS) p = plan_pg_scan_sums(capacity);
    else return CANNY_HIP_ERR_INVALID;
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// Host-only: the launch plans of the capped chamfer launches for a full chunk of the batch.
int canny_hip_selftest_chamfer_plan(int which, int n_frames, int height, int width, int n_templates, int with_scores,
                                    unsigned long long *out)
{
    if (!out || check_dims(height, width, n_frames) || n_templates < 1 || n_templates > CANNY_HIP_CHAMFER_MAX_TEMPLATES ||
        (long long)height * width * n_templates >= 0x80000000LL)
        return CANNY_HIP_ERR_INVALID;
    const int chunk = chamfer_chunk_frames(n_frames, height, width, n_templates, with_scores != 0);
    LaunchPlan p;
    if (which == CANNY_HIP_CHAMFER_PLAN_COST) p = plan_chamfer_cost((unsigned long long)chunk * height * width);
    else if (which == CANNY_HIP_CHAMFER_PLAN_CELLS) p = plan_chamfer_cells((unsigned long long)height * width * n_templates);
    else return CANNY_HIP_ERR_INVALID;
    store_plan(out, p);
    out[5] = (unsigned long long)chunk;
    return CANNY_HIP_OK;
}

int canny_hip_selftest_chamfer_bands(const int *offsets, const short *points, int n_templates, int t, int *out)
{
    if (!out || t < 0) return CANNY_HIP_ERR_INVALID;
    ChamferLayout lay;
    const int rc = chamfer_build_layout(offsets, points, n_templates, lay);
    if (rc) return rc;
    if (t >= n_templates) return CANNY_HIP_ERR_INVALID;
    const int cols = kChamferTileX + lay.boxes[(size_t)t].max_x - lay.boxes[(size_t)t].min_x;
    out[0] = lay.band_offsets[(size_t)t + 1] - lay.band_offsets[(size_t)t];
    out[1] = 0;
    for (int b = lay.band_offsets[(size_t)t]; b < lay.band_offsets[(size_t)t + 1]; b++)
        out[1] = std::max(out[1], lay.bands[(size_t)b].rows * cols);
    out[2] = lay.max_elems;
    out[3] = chamfer_auto_route(lay);
    return CANNY_HIP_OK;
}

// ---- corners, Harris / Shi-Tomasi (canny_corners.hip) ------------------------------
} // extern "C"

namespace {

struct CornerOut {
    long long *d_corners;
    int *d_counts, *d_cand_counts;
    long long *d_max_response, *d_response;
};

// THE check of the corner arguments; needs no device and writes nothing
int corners_check(int height, int width, int n_frames, const CornerArgs &a, const CornerOut &out)
{
    const bool mode_ok = a.mode == CANNY_HIP_CORNERS_MIN_EIGEN || a.mode == CANNY_HIP_CORNERS_HARRIS;
    if (!mode_ok || (a.block != 3 && a.block != 5 && a.block != 7) || a.k_q8 < 0 || a.k_q8 > CANNY_HIP_CORNERS_MAX_K_Q8 ||
        (a.mode == CANNY_HIP_CORNERS_MIN_EIGEN && a.k_q8 != 0) || a.quality_q16 < 0 || a.quality_q16 > 65536 ||
        a.min_response < 0 || a.min_dist < 0 || a.corners_max < 1 || !out.d_corners || !out.d_counts ||
        ((uintptr_t)out.d_corners & 7) || ((uintptr_t)out.d_response & 7) || ((uintptr_t)out.d_max_response & 7) ||
        height < 2 || width < 2 || n_frames < 1)
        return CANNY_HIP_ERR_INVALID;
    if ((long long)height * width >= 0x80000000LL || n_frames > 65535 || a.corners_max > kHoughMaxLines || height > 65535 ||
        width > 65535)
        return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// The corners of n frames of a device plane, queued on the context's stream, chunk of frames by chunk of frames.
int dev_corners(canny_hip_ctx *ctx, const void *plane, bool plane_u8, int n, int h, int w, const CornerArgs &a,
                const CornerOut &out)
{
    const size_t hw = (size_t)h * w, px_bytes = plane_u8 ? 1 : 2;
    const int chunk = std::min(n, kCornersChunk);
    HIP_TRY(ctx, ctx->corners_ws.ensure(corners_ws_bytes(chunk, a.corners_max, h, w)));
    void *ws = ctx->corners_ws.p;
    const int part = canny_hip_ctx::kProfCorners;
    for (int f0 = 0; f0 < n; f0 += chunk) {
        const int nf = std::min(chunk, n - f0);
        const void *pl = (const char *)plane + (size_t)f0 * hw * px_bytes;
        {
            StageTimer tm(ctx, part + CANNY_HIP_CORNER_PART_MAX);
            HIP_TRY(ctx, launch_corners_max(pl, plane_u8, nf, h, w, a, ws,
                                            out.d_response ? out.d_response + (size_t)f0 * hw : nullptr, ctx->stream));
        }
        {
            StageTimer tm(ctx, part + CANNY_HIP_CORNER_PART_CANDIDATES);
            HIP_TRY(ctx, launch_corners_candidates(pl, plane_u8, nf, h, w, a, ws,
                                                   out.d_cand_counts ? out.d_cand_counts + f0 : nullptr,
                                                   out.d_max_response ? out.d_max_response + f0 : nullptr, ctx->stream));
        }
        {
            StageTimer tm(ctx, part + CANNY_HIP_CORNER_PART_COLLECT);
            HIP_TRY(ctx, launch_corners_collect(pl, plane_u8, nf, h, w, a, ws, ctx->stream));
        }
        {
            StageTimer tm(ctx, part + CANNY_HIP_CORNER_PART_ACCEPT);
            HIP_TRY(ctx, launch_corners_accept(nf, h, w, a, ws,
                                               out.d_corners + (size_t)f0 * a.corners_max * CANNY_HIP_CORNER_WORDS,
                                               out.d_counts + f0, ctx->stream));
        }
    }
    return CANNY_HIP_OK;
}

} // namespace

extern "C" {

int canny_hip_dev_canny_corners(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                int height, int width, int n_frames, short *d_edges, int mode, int block, int k_q8,
                                int quality_q16, long long min_response, int min_dist, int corners_max,
                                long long *d_corners, int *d_counts, int *d_cand_counts, long long *d_max_response,
                                long long *d_response)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_img) return CANNY_HIP_ERR_INVALID;
    const CornerArgs a{mode, block, k_q8, quality_q16, min_response, min_dist, corners_max};
    const CornerOut out{d_corners, d_counts, d_cand_counts, d_max_response, d_response};
    if ((rc = corners_check(height, width, n_frames, a, out))) return rc;
    // the corners come from the smoothed plane, not the map: dev_canny leaves the whole batch's in ctx->smoothed, as bytes
    // iff last_canny_u8
    const uint64_t *strong_unused;
    if ((rc = dev_canny_map(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, &strong_unused))) return rc;
    return dev_corners(ctx, ctx->smoothed.p, ctx->last_canny_u8 != 0, n_frames, height, width, a, out);
}

int canny_hip_dev_corners_plane(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int height, int width,
                                int mode, int block, int k_q8, int quality_q16, long long min_response, int min_dist,
                                int corners_max, long long *d_corners, int *d_counts, int *d_cand_counts,
                                long long *d_max_response, long long *d_response)
{
    int rc = bind(ctx);
    if (rc) return rc;
    const CornerArgs a{mode, block, k_q8, quality_q16, min_response, min_dist, corners_max};
    const CornerOut out{d_corners, d_counts, d_cand_counts, d_max_response, d_response};
    if ((rc = corners_check(height, width, n_frames, a, out))) return rc;
    const void *plane = d_plane;
    bool plane_u8 = true;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, height, width) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        plane = ctx->smoothed.p;
        plane_u8 = ctx->last_canny_u8 != 0;
    }
    if ((rc = finish_pending(ctx))) return rc;
    return dev_corners(ctx, plane, plane_u8, n_frames, height, width, a, out);
}

int canny_hip_canny_corners(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                            int max_val, int height, int width, int mode, int block, int k_q8, int quality_q16,
                            long long min_response, int min_dist, int corners_max, long long *corners, int *counts,
                            int *cand_counts, long long *max_response)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs) return CANNY_HIP_ERR_INVALID;
    const CornerArgs a{mode, block, k_q8, quality_q16, min_response, min_dist, corners_max};
    if ((rc = corners_check(height, width, n_frames, a, CornerOut{corners, counts, nullptr, nullptr, nullptr}))) return rc;
    const size_t slots = (size_t)n_frames * corners_max;
    // one staging block: records (4 long long per slot) | maxima | counts | candidate counts
    HIP_TRY(ctx, ctx->io[1].ensure((slots * CANNY_HIP_CORNER_WORDS + (size_t)n_frames) * sizeof(long long) +
                                   2 * (size_t)n_frames * sizeof(int)));
    long long *d_rec = (long long *)ctx->io[1].p, *d_max = d_rec + slots * CANNY_HIP_CORNER_WORDS;
    int *d_cnt = (int *)(d_max + n_frames);
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_corners(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width,
                                          n_frames, nullptr, mode, block, k_q8, quality_q16, min_response, min_dist,
                                          corners_max, d_rec, d_cnt, d_cnt + n_frames, d_max, nullptr)))
        return rc;
    std::vector<long long> words((size_t)n_frames * 2); // maxima | counts, candidate counts (as they lie on the device)
    if ((rc = d2h_sync(ctx, words.data(), d_max, words.size() * sizeof(long long)))) return rc;
    const int *cnt = (const int *)(words.data() + n_frames);
    for (int f = 0; f < n_frames; f++) { // only the filled slots of each frame come down
        const size_t k = (size_t)cnt[f], at = (size_t)f * corners_max * CANNY_HIP_CORNER_WORDS;
        if (k) HIP_TRY(ctx, hipMemcpyAsync(corners + at, d_rec + at, k * CANNY_HIP_CORNER_WORDS * sizeof(long long),
                                          hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(counts, cnt, (size_t)n_frames * sizeof(int));
    if (cand_counts) std::memcpy(cand_counts, cnt + n_frames, (size_t)n_frames * sizeof(int));
    if (max_response) std::memcpy(max_response, words.data(), (size_t)n_frames * sizeof(long long));
    return CANNY_HIP_OK;
}

// canny_hip_corners_from_plane and canny_hip_corner_response_of, the rule in plain C++, live in canny_corners_host.cpp.

int canny_hip_dev_corners_arith(canny_hip_ctx *ctx, const int *d_sums, size_t n, int mode, int k_q8, long long *d_r)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_sums || !d_r || !n || ((uintptr_t)d_r & 7) ||
        (mode != CANNY_HIP_CORNERS_MIN_EIGEN && mode != CANNY_HIP_CORNERS_HARRIS) || k_q8 < 0 ||
        k_q8 > CANNY_HIP_CORNERS_MAX_K_Q8 || (mode == CANNY_HIP_CORNERS_MIN_EIGEN && k_q8 != 0))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, launch_corners_arith(d_sums, n, mode, k_q8, d_r, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_corners_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfCorners, CANNY_HIP_CORNER_PARTS, part, total_ms, launches);
}

// Host-only: the launch plans of the capped launches of the corners.
int canny_hip_selftest_corners_plan(int which, int n_frames, int height, int width, unsigned long long n,
                                    unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    LaunchPlan p;
    if (which == CANNY_HIP_CORNERS_PLAN_TILES) {
        if (height < 2 || width < 2 || check_dims(height, width, n_frames)) return CANNY_HIP_ERR_INVALID;
        p = plan_corners_tiles(height, width);
        out[5] = (unsigned long long)std::min(n_frames, kCornersChunk);
    } else if (which == CANNY_HIP_CORNERS_PLAN_ARITH) {
        if (!n) return CANNY_HIP_ERR_INVALID;
        p = plan_corners_arith((size_t)n);
        out[5] = 0;
    } else {
        return CANNY_HIP_ERR_INVALID;
    }
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// ---- corner descriptors and Hamming matching (canny_descriptors.hip) ------------------------------
} // extern "C"

namespace {

// THE check of the descriptor arguments; needs no device and writes nothing
int descriptors_check(int height, int width, int n_frames, int corners_max, int options, const void *d_corners,
                      const void *d_counts, const void *d_desc, const void *d_meta)
{
    if ((options & ~CANNY_HIP_DESC_STEERED) || corners_max < 1 || !d_corners || !d_counts || !d_desc || !d_meta ||
        ((uintptr_t)d_corners & 7) || ((uintptr_t)d_desc & 7) || height < 2 || width < 2 || n_frames < 1)
        return CANNY_HIP_ERR_INVALID;
    if ((long long)height * width >= 0x80000000LL || n_frames > 65535 || corners_max > kHoughMaxLines)
        return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

int dev_describe(canny_hip_ctx *ctx, const void *plane, bool plane_u8, int n, int h, int w, const long long *d_corners,
                 const int *d_counts, int corners_max, int options, unsigned long long *d_desc, int *d_meta)
{
    StageTimer tm(ctx, canny_hip_ctx::kProfDescriptors + CANNY_HIP_DESC_PART_DESCRIBE);
    HIP_TRY(ctx, launch_desc_describe(plane, plane_u8, n, h, w, d_corners, d_counts, corners_max,
                                      (options & CANNY_HIP_DESC_STEERED) != 0, d_desc, d_meta, ctx->stream));
    return CANNY_HIP_OK;
}

} // namespace

extern "C" {

int canny_hip_dev_canny_corner_descriptors(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                           int max_val, int height, int width, int n_frames, short *d_edges, int mode,
                                           int block, int k_q8, int quality_q16, long long min_response, int min_dist,
                                           int corners_max, long long *d_corners, int *d_counts, int *d_cand_counts,
                                           long long *d_max_response, long long *d_response, int desc_options,
                                           unsigned long long *d_desc, int *d_meta)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = descriptors_check(height, width, n_frames, corners_max, desc_options, d_corners, d_counts, d_desc, d_meta)))
        return rc;
    // the corners call checks its own arguments before it queues anything
    if ((rc = canny_hip_dev_canny_corners(ctx, d_img, sigma, min_val, max_val, height, width, n_frames, d_edges, mode, block,
                                          k_q8, quality_q16, min_response, min_dist, corners_max, d_corners, d_counts,
                                          d_cand_counts, d_max_response, d_response)))
        return rc;
    return dev_describe(ctx, ctx->smoothed.p, ctx->last_canny_u8 != 0, n_frames, height, width, d_corners, d_counts,
                        corners_max, desc_options, d_desc, d_meta);
}

int canny_hip_dev_corner_descriptors(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int height, int width,
                                     const long long *d_corners, const int *d_counts, int corners_max, int desc_options,
                                     unsigned long long *d_desc, int *d_meta)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = descriptors_check(height, width, n_frames, corners_max, desc_options, d_corners, d_counts, d_desc, d_meta)))
        return rc;
    const void *plane = d_plane;
    bool plane_u8 = true;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, height, width) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        plane = ctx->smoothed.p;
        plane_u8 = ctx->last_canny_u8 != 0;
    }
    if ((rc = finish_pending(ctx))) return rc;
    return dev_describe(ctx, plane, plane_u8, n_frames, height, width, d_corners, d_counts, corners_max, desc_options,
                        d_desc, d_meta);
}

int canny_hip_canny_corner_descriptors(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma,
                                       int min_val, int max_val, int height, int width, int mode, int block, int k_q8,
                                       int quality_q16, long long min_response, int min_dist, int corners_max,
                                       int desc_options, long long *corners, int *counts, unsigned long long *desc,
                                       int *meta)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs) return CANNY_HIP_ERR_INVALID;
    if ((rc = descriptors_check(height, width, n_frames, corners_max, desc_options, corners, counts, desc, meta))) return rc;
    const CornerArgs a{mode, block, k_q8, quality_q16, min_response, min_dist, corners_max};
    if ((rc = corners_check(height, width, n_frames, a, CornerOut{corners, counts, nullptr, nullptr, nullptr}))) return rc;
    const size_t slots = (size_t)n_frames * corners_max;
    // one staging block: records (4 long long per slot) | descriptors (4 words per slot) | meta | counts
    HIP_TRY(ctx, ctx->io[1].ensure(slots * (CANNY_HIP_CORNER_WORDS * sizeof(long long) +
                                            CANNY_HIP_DESC_WORDS * sizeof(unsigned long long) + sizeof(int)) +
                                   (size_t)n_frames * sizeof(int)));
    long long *d_rec = (long long *)ctx->io[1].p;
    unsigned long long *d_desc = (unsigned long long *)(d_rec + slots * CANNY_HIP_CORNER_WORDS);
    int *d_meta = (int *)(d_desc + slots * CANNY_HIP_DESC_WORDS), *d_cnt = d_meta + slots;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_corner_descriptors(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val,
                                                     height, width, n_frames, nullptr, mode, block, k_q8, quality_q16,
                                                     min_response, min_dist, corners_max, d_rec, d_cnt, nullptr, nullptr,
                                                     nullptr, desc_options, d_desc, d_meta)))
        return rc;
    std::vector<int> cnt((size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_cnt, cnt.size() * sizeof(int)))) return rc;
    for (int f = 0; f < n_frames; f++) { // only the filled slots of each frame come down
        const size_t k = (size_t)cnt[f], at = (size_t)f * corners_max;
        if (!k) continue;
        HIP_TRY(ctx, hipMemcpyAsync(corners + at * CANNY_HIP_CORNER_WORDS, d_rec + at * CANNY_HIP_CORNER_WORDS,
                                    k * CANNY_HIP_CORNER_WORDS * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(desc + at * CANNY_HIP_DESC_WORDS, d_desc + at * CANNY_HIP_DESC_WORDS,
                                    k * CANNY_HIP_DESC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(meta + at, d_meta + at, k * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(counts, cnt.data(), (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

// canny_hip_corner_descriptors_from_plane, canny_hip_descriptor_pattern and canny_hip_match_descriptors, the rule in plain
// C++, live in canny_descriptors_host.cpp.

int canny_hip_dev_match_descriptors(canny_hip_ctx *ctx, const unsigned long long *d_q_desc, const int *d_q_counts,
                                    int n_q_frames, int stride_q, const unsigned long long *d_t_desc, const int *d_t_counts,
                                    int n_t_frames, int stride_t, const int *pairs, int n_pairs, int max_distance,
                                    int ratio_q8, int options, int *d_matches, int *d_pair_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_q_desc || !d_q_counts || !d_t_desc || !d_t_counts || !pairs || !d_matches || !d_pair_counts || n_q_frames < 1 ||
        n_t_frames < 1 || stride_q < 1 || stride_t < 1 || n_pairs < 1 || max_distance < 0 ||
        max_distance > CANNY_HIP_DESC_BITS || ratio_q8 < 0 || ratio_q8 > 256 || (options & ~CANNY_HIP_MATCH_CROSS_CHECK) ||
        ((uintptr_t)d_q_desc & 7) || ((uintptr_t)d_t_desc & 7))
        return CANNY_HIP_ERR_INVALID;
    if (stride_q > kHoughMaxLines || stride_t > kHoughMaxLines || n_q_frames > 65535 || n_t_frames > 65535 ||
        n_pairs > CANNY_HIP_MATCH_MAX_PAIRS)
        return CANNY_HIP_ERR_UNSUPPORTED;
    for (int p = 0; p < n_pairs; p++)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_q_frames || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_t_frames)
            return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    // the workspace: the pairs | per (pair, train slot) its best query
    const size_t pair_ints = 2 * (size_t)n_pairs;
    HIP_TRY(ctx, ctx->desc_ws.ensure((pair_ints + (size_t)n_pairs * stride_t) * sizeof(int)));
    int *d_pairs = (int *)ctx->desc_ws.p, *d_back = d_pairs + pair_ints;
    ctx->desc_pairs.assign(pairs, pairs + pair_ints);
    HIP_TRY(ctx, hipMemcpyAsync(d_pairs, ctx->desc_pairs.data(), pair_ints * sizeof(int), hipMemcpyHostToDevice,
                                ctx->stream));
    const int part = canny_hip_ctx::kProfDescriptors;
    {
        StageTimer tm(ctx, part + CANNY_HIP_DESC_PART_MATCH);
        HIP_TRY(ctx, launch_desc_match(d_q_desc, d_q_counts, stride_q, d_t_desc, d_t_counts, stride_t, d_pairs, n_pairs,
                                       false, d_matches, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_DESC_PART_REVERSE);
        HIP_TRY(ctx, launch_desc_match(d_t_desc, d_t_counts, stride_t, d_q_desc, d_q_counts, stride_q, d_pairs, n_pairs,
                                       true, d_back, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_DESC_PART_FINALIZE);
        HIP_TRY(ctx, launch_desc_finalize(d_q_counts, stride_q, stride_t, d_pairs, n_pairs, d_back, max_distance, ratio_q8,
                                          (options & CANNY_HIP_MATCH_CROSS_CHECK) != 0, d_matches, d_pair_counts,
                                          ctx->stream));
    }
    return CANNY_HIP_OK;
}

int canny_hip_descriptors_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfDescriptors, CANNY_HIP_DESC_PARTS, part, total_ms, launches);
}

// Host-only: the launch plans of the capped launches of the descriptors and their matching.
int canny_hip_selftest_descriptors_plan(int which, unsigned long long n, int stride, unsigned long long *out)
{
    if (!out || !n || stride < 1 || stride > kHoughMaxLines) return CANNY_HIP_ERR_INVALID;
    LaunchPlan p;
    if (which == CANNY_HIP_DESCRIPTORS_PLAN_DESCRIBE) {
        if (n > 65535) return CANNY_HIP_ERR_INVALID;
        p = plan_desc_slots(n * (unsigned long long)stride);
    } else if (which == CANNY_HIP_DESCRIPTORS_PLAN_MATCH) {
        if (n > CANNY_HIP_MATCH_MAX_PAIRS) return CANNY_HIP_ERR_INVALID;
        p = plan_desc_match(n, stride);
    } else {
        return CANNY_HIP_ERR_INVALID;
    }
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// ---- frame-to-frame motion from the corner matches (canny_motion.hip) -----------------------------
// canny_hip_estimate_motion, the rule in plain C++, lives in canny_motion_host.cpp.

int canny_hip_dev_estimate_motion(canny_hip_ctx *ctx, const long long *d_q_corners, const int *d_q_counts, int n_q_frames,
                                  int stride_q, const long long *d_t_corners, const int *d_t_counts, int n_t_frames,
                                  int stride_t, const int *pairs, int n_pairs, const int *d_matches, int model, int thr_q4,
                                  int hypotheses, unsigned seed, long long *d_motion, int *d_inlier)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_q_corners || !d_q_counts || !d_t_corners || !d_t_counts || !pairs || !d_matches || !d_motion || n_q_frames < 1 ||
        n_t_frames < 1 || stride_q < 1 || stride_t < 1 || n_pairs < 1 || model < CANNY_HIP_MOTION_TRANSLATION ||
        model > CANNY_HIP_MOTION_AFFINE || thr_q4 < 0 || thr_q4 > 4095 || hypotheses < 1 || ((uintptr_t)d_q_corners & 7) ||
        ((uintptr_t)d_t_corners & 7) || ((uintptr_t)d_motion & 7))
        return CANNY_HIP_ERR_INVALID;
    if (stride_q > kHoughMaxLines || stride_t > kHoughMaxLines || n_q_frames > 65535 || n_t_frames > 65535 ||
        n_pairs > CANNY_HIP_MATCH_MAX_PAIRS || hypotheses > CANNY_HIP_MOTION_MAX_HYPOTHESES)
        return CANNY_HIP_ERR_UNSUPPORTED;
    for (int p = 0; p < n_pairs; p++)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_q_frames || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_t_frames)
            return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    HIP_TRY(ctx, ctx->motion_ws.ensure(motion_workspace(nullptr, n_pairs, stride_q, hypotheses).bytes));
    const MotionWs w = motion_workspace(ctx->motion_ws.p, n_pairs, stride_q, hypotheses);
    ctx->motion_pairs.assign(pairs, pairs + 2 * (size_t)n_pairs);
    HIP_TRY(ctx, hipMemcpyAsync(w.pairs, ctx->motion_pairs.data(), 2 * (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice,
                                ctx->stream));
    const int part = canny_hip_ctx::kProfMotion;
    {
        StageTimer tm(ctx, part + CANNY_HIP_MOTION_PART_GATHER);
        HIP_TRY(ctx, launch_motion_gather(d_q_corners, d_q_counts, stride_q, d_t_corners, d_t_counts, stride_t, n_pairs,
                                          d_matches, w, d_inlier, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_MOTION_PART_SCORE);
        HIP_TRY(ctx, launch_motion_score(stride_q, n_pairs, model, thr_q4, hypotheses, seed, w, ctx->stream));
    }
    {
        StageTimer tm(ctx, part + CANNY_HIP_MOTION_PART_REFIT);
        HIP_TRY(ctx, launch_motion_refit(stride_q, n_pairs, model, thr_q4, hypotheses, seed, w, d_motion, d_inlier,
                                         ctx->stream));
    }
    return CANNY_HIP_OK;
}

int canny_hip_canny_motion(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int mode, int block, int k_q8, int quality_q16,
                           long long min_response, int min_dist, int corners_max, int desc_options, const int *pairs,
                           int n_pairs, int max_distance, int ratio_q8, int match_options, int model, int thr_q4,
                           int hypotheses, unsigned seed, long long *motion, long long *corners, int *counts, int *matches,
                           int *inlier)
{
    int rc = bind(ctx);
    if (rc) return rc;
    // every check of the chained calls, before anything is uploaded or queued
    if (!imgs || !pairs || !motion || n_pairs < 1 || (corners == nullptr) != (counts == nullptr) || max_distance < 0 ||
        max_distance > CANNY_HIP_DESC_BITS || ratio_q8 < 0 || ratio_q8 > 256 || (match_options & ~CANNY_HIP_MATCH_CROSS_CHECK) ||
        model < CANNY_HIP_MOTION_TRANSLATION || model > CANNY_HIP_MOTION_AFFINE || thr_q4 < 0 || thr_q4 > 4095 ||
        hypotheses < 1 || ((uintptr_t)motion & 7) || ((uintptr_t)corners & 7))
        return CANNY_HIP_ERR_INVALID;
    // the descriptor check wants its four pointers: the outputs that stay on the device stand in
    if ((rc = descriptors_check(height, width, n_frames, corners_max, desc_options, motion, motion, motion, motion))) return rc;
    const CornerArgs a{mode, block, k_q8, quality_q16, min_response, min_dist, corners_max};
    long long *probe_rec = motion;
    int *probe_cnt = (int *)motion;
    if ((rc = corners_check(height, width, n_frames, a, CornerOut{probe_rec, probe_cnt, nullptr, nullptr, nullptr}))) return rc;
    if (n_pairs > CANNY_HIP_MATCH_MAX_PAIRS || hypotheses > CANNY_HIP_MOTION_MAX_HYPOTHESES) return CANNY_HIP_ERR_UNSUPPORTED;
    for (int p = 0; p < n_pairs; p++)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_frames || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_frames)
            return CANNY_HIP_ERR_INVALID;
    const size_t slots = (size_t)n_frames * corners_max, pslots = (size_t)n_pairs * corners_max;
    // one staging block: records | descriptors | motion records | meta | counts | matches | pair counts | inlier flags
    HIP_TRY(ctx, ctx->io[1].ensure(slots * (CANNY_HIP_CORNER_WORDS * sizeof(long long) +
                                            CANNY_HIP_DESC_WORDS * sizeof(unsigned long long) + sizeof(int)) +
                                   (size_t)n_pairs * CANNY_HIP_MOTION_WORDS * sizeof(long long) +
                                   (size_t)n_frames * sizeof(int) + pslots * (CANNY_HIP_MATCH_WORDS + 1) * sizeof(int) +
                                   (size_t)n_pairs * sizeof(int)));
    long long *d_rec = (long long *)ctx->io[1].p;
    unsigned long long *d_desc = (unsigned long long *)(d_rec + slots * CANNY_HIP_CORNER_WORDS);
    long long *d_motion = (long long *)(d_desc + slots * CANNY_HIP_DESC_WORDS);
    int *d_meta = (int *)(d_motion + (size_t)n_pairs * CANNY_HIP_MOTION_WORDS), *d_cnt = d_meta + slots;
    int *d_matches = d_cnt + n_frames, *d_pc = d_matches + pslots * CANNY_HIP_MATCH_WORDS, *d_in = d_pc + n_pairs;
    if ((rc = h2d(ctx, ctx->io[0], imgs, npx(height, width, n_frames)))) return rc;
    if ((rc = canny_hip_dev_canny_corner_descriptors(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val,
                                                     height, width, n_frames, nullptr, mode, block, k_q8, quality_q16,
                                                     min_response, min_dist, corners_max, d_rec, d_cnt, nullptr, nullptr,
                                                     nullptr, desc_options, d_desc, d_meta)))
        return rc;
    if ((rc = canny_hip_dev_match_descriptors(ctx, d_desc, d_cnt, n_frames, corners_max, d_desc, d_cnt, n_frames,
                                              corners_max, pairs, n_pairs, max_distance, ratio_q8, match_options, d_matches,
                                              d_pc)))
        return rc;
    if ((rc = canny_hip_dev_estimate_motion(ctx, d_rec, d_cnt, n_frames, corners_max, d_rec, d_cnt, n_frames, corners_max,
                                            pairs, n_pairs, d_matches, model, thr_q4, hypotheses, seed, d_motion,
                                            inlier ? d_in : nullptr)))
        return rc;
    std::vector<int> cnt((size_t)n_frames);
    if ((rc = d2h_sync(ctx, cnt.data(), d_cnt, cnt.size() * sizeof(int)))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(motion, d_motion, (size_t)n_pairs * CANNY_HIP_MOTION_WORDS * sizeof(long long),
                                hipMemcpyDeviceToHost, ctx->stream));
    if (corners)
        for (int f = 0; f < n_frames; f++) { // only the filled slots of each frame come down
            const size_t k = (size_t)cnt[f], at = (size_t)f * corners_max;
            if (k)
                HIP_TRY(ctx, hipMemcpyAsync(corners + at * CANNY_HIP_CORNER_WORDS, d_rec + at * CANNY_HIP_CORNER_WORDS,
                                            k * CANNY_HIP_CORNER_WORDS * sizeof(long long), hipMemcpyDeviceToHost,
                                            ctx->stream));
        }
    for (int p = 0; p < n_pairs; p++) { // of every pair the slots below the query's count
        const size_t k = (size_t)cnt[pairs[2 * p]], at = (size_t)p * corners_max;
        if (!k) continue;
        if (matches)
            HIP_TRY(ctx, hipMemcpyAsync(matches + at * CANNY_HIP_MATCH_WORDS, d_matches + at * CANNY_HIP_MATCH_WORDS,
                                        k * CANNY_HIP_MATCH_WORDS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (inlier)
            HIP_TRY(ctx, hipMemcpyAsync(inlier + at, d_in + at, k * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (counts) std::memcpy(counts, cnt.data(), (size_t)n_frames * sizeof(int));
    return CANNY_HIP_OK;
}

int canny_hip_motion_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfMotion, CANNY_HIP_MOTION_PARTS, part, total_ms, launches);
}

// Host-only: the launch plans of the capped launches of the motion estimate.
int canny_hip_selftest_motion_plan(int which, unsigned long long n_pairs, int hypotheses, unsigned long long *out)
{
    if (!out || !n_pairs || n_pairs > CANNY_HIP_MATCH_MAX_PAIRS || hypotheses < 1 ||
        hypotheses > CANNY_HIP_MOTION_MAX_HYPOTHESES)
        return CANNY_HIP_ERR_INVALID;
    LaunchPlan p;
    if (which == CANNY_HIP_MOTION_PLAN_GATHER || which == CANNY_HIP_MOTION_PLAN_REFIT)
        p = plan_motion_pairs(n_pairs);
    else if (which == CANNY_HIP_MOTION_PLAN_SCORE)
        p = plan_motion_score(n_pairs, hypotheses);
    else
        return CANNY_HIP_ERR_INVALID;
    store_plan(out, p);
    return CANNY_HIP_OK;
}

// ---- frame alignment: the motions chained, frames warped (canny_warp.hip) --------------------------
// canny_hip_compose_motion and canny_hip_warp_frames, the rules in plain C++, live in canny_warp_host.cpp.

int canny_hip_dev_compose_motion(canny_hip_ctx *ctx, const long long *d_motion, int n_pairs, int first_frame,
                                 long long *d_xforms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (n_pairs < 0 || first_frame < 0 || !d_xforms || (n_pairs > 0 && !d_motion) || ((uintptr_t)d_motion & 7) ||
        ((uintptr_t)d_xforms & 7))
        return CANNY_HIP_ERR_INVALID;
    if (n_pairs > 65535) return CANNY_HIP_ERR_UNSUPPORTED;
    if ((rc = finish_pending(ctx))) return rc;
    StageTimer tm(ctx, canny_hip_ctx::kProfWarp + CANNY_HIP_WARP_PART_COMPOSE);
    HIP_TRY(ctx, launch_warp_compose(d_motion, n_pairs, first_frame, d_xforms, ctx->stream));
    return CANNY_HIP_OK;
}

namespace {
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// every check of the warp but the pointers
int warp_check(int n_src, int src_h, int src_w, int n_out, int out_h, int out_w, int interp, int border)
{
    if (n_src < 1 || n_out < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 ||
        (interp != CANNY_HIP_WARP_NEAREST && interp != CANNY_HIP_WARP_BILINEAR) || border < 0 || border > 255)
        return CANNY_HIP_ERR_INVALID;
    if (src_h > 32768 || src_w > 32768 || out_h > 32768 || out_w > 32768 || (long long)src_h * src_w >= (1ll << 31) ||
        (long long)out_h * out_w >= (1ll << 31) || n_src > 65535 || n_out > 65535)
        return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_warp_frames(canny_hip_ctx *ctx, const unsigned char *d_src, int n_src, int src_h, int src_w,
                              const long long *d_xforms, int n_out, int out_h, int out_w, int interp, int border,
                              unsigned char *d_out, unsigned char *d_valid_bits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_src || !d_xforms || !d_out || ((uintptr_t)d_xforms & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = warp_check(n_src, src_h, src_w, n_out, out_h, out_w, interp, border))) return rc;
    const size_t src_bytes = npx(src_h, src_w, n_src), out_bytes = npx(out_h, out_w, n_out);
    const size_t valid_bytes = npx(out_h, (out_w + 7) / 8, n_out);
    if (ranges_overlap(d_src, src_bytes, d_out, out_bytes) ||
        (d_valid_bits && (ranges_overlap(d_src, src_bytes, d_valid_bits, valid_bytes) ||
                          ranges_overlap(d_out, out_bytes, d_valid_bits, valid_bytes))))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    StageTimer tm(ctx, canny_hip_ctx::kProfWarp + CANNY_HIP_WARP_PART_WARP);
    HIP_TRY(ctx, launch_warp_frames(d_src, n_src, src_h, src_w, d_xforms, n_out, out_h, out_w, interp, border,
                                    ctx->warp_route, d_out, d_valid_bits, ctx->stream));
    return CANNY_HIP_OK;
}

namespace {
// What the alignment chain leaves on the device, all inside the staging block io[1]: canny_hip_canny_align brings it down,
// canny_hip_canny_background goes on from it.  extra: extra_bytes behind the valid bits, 16-byte aligned.
struct AlignDev {
    unsigned char *aligned = nullptr, *valid = nullptr, *extra = nullptr;
    long long *xf = nullptr, *motion = nullptr;
    size_t frame_bytes = 0, valid_bytes = 0;
    int n_pairs = 0;
};

// The chain of canny_hip_canny_align up to the warp.  xforms, motion: the caller's host buffers, only checked here.
int align_on_device(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                    int height, int width, int mode, int block, int k_q8, int quality_q16, long long min_response,
                    int min_dist, int corners_max, int desc_options, int max_distance, int ratio_q8, int match_options,
                    int model, int thr_q4, int hypotheses, unsigned seed, int interp, int border, long long *xforms,
                    const long long *motion, bool want_valid, size_t extra_bytes, AlignDev &dev)
{
    int rc;
    // every check of the chained calls, before anything is uploaded or queued
    if (!imgs || !xforms || max_distance < 0 || max_distance > CANNY_HIP_DESC_BITS || ratio_q8 < 0 ||
        ratio_q8 > 256 || (match_options & ~CANNY_HIP_MATCH_CROSS_CHECK) || model < CANNY_HIP_MOTION_TRANSLATION ||
        model > CANNY_HIP_MOTION_AFFINE || thr_q4 < 0 || thr_q4 > 4095 || hypotheses < 1 || ((uintptr_t)xforms & 7) ||
        ((uintptr_t)motion & 7))
        return CANNY_HIP_ERR_INVALID;
    // the descriptor check wants its four pointers: the outputs that stay on the device stand in
    if ((rc = descriptors_check(height, width, n_frames, corners_max, desc_options, xforms, xforms, xforms, xforms))) return rc;
    const CornerArgs a{mode, block, k_q8, quality_q16, min_response, min_dist, corners_max};
    if ((rc = corners_check(height, width, n_frames, a, CornerOut{xforms, (int *)xforms, nullptr, nullptr, nullptr}))) return rc;
    if ((rc = warp_check(n_frames, height, width, n_frames, height, width, interp, border))) return rc;
    if (hypotheses > CANNY_HIP_MOTION_MAX_HYPOTHESES) return CANNY_HIP_ERR_UNSUPPORTED;
    const int n_pairs = n_frames - 1;
    std::vector<int> pairs(2 * (size_t)n_pairs);
    for (int p = 0; p < n_pairs; p++) pairs[2 * p] = p, pairs[2 * p + 1] = p + 1;
    const size_t slots = (size_t)n_frames * corners_max, pslots = (size_t)n_pairs * corners_max;
    const size_t frame_bytes = npx(height, width, n_frames), valid_bytes = npx(height, (width + 7) / 8, n_frames);
    // one staging block: records | descriptors | motion records | transform records | meta | counts | matches | pair counts |
    // aligned frames | valid bits | what the caller asked for behind them
    HIP_TRY(ctx, ctx->io[1].ensure(slots * (CANNY_HIP_CORNER_WORDS * sizeof(long long) +
                                            CANNY_HIP_DESC_WORDS * sizeof(unsigned long long) + sizeof(int)) +
                                   (size_t)n_pairs * CANNY_HIP_MOTION_WORDS * sizeof(long long) +
                                   (size_t)n_frames * CANNY_HIP_XFORM_WORDS * sizeof(long long) +
                                   (size_t)n_frames * sizeof(int) + pslots * CANNY_HIP_MATCH_WORDS * sizeof(int) +
                                   (size_t)n_pairs * sizeof(int) + 16 + frame_bytes + valid_bytes + 16 + extra_bytes));
    long long *d_rec = (long long *)ctx->io[1].p;
    unsigned long long *d_desc = (unsigned long long *)(d_rec + slots * CANNY_HIP_CORNER_WORDS);
    long long *d_motion = (long long *)(d_desc + slots * CANNY_HIP_DESC_WORDS);
    long long *d_xf = d_motion + (size_t)n_pairs * CANNY_HIP_MOTION_WORDS;
    int *d_meta = (int *)(d_xf + (size_t)n_frames * CANNY_HIP_XFORM_WORDS), *d_cnt = d_meta + slots;
    int *d_matches = d_cnt + n_frames, *d_pc = d_matches + pslots * CANNY_HIP_MATCH_WORDS;
    unsigned char *d_aligned = (unsigned char *)(((uintptr_t)(d_pc + n_pairs) + 15) & ~(uintptr_t)15);
    unsigned char *d_valid = d_aligned + frame_bytes;
    dev.aligned = d_aligned, dev.valid = d_valid, dev.xf = d_xf, dev.motion = d_motion, dev.n_pairs = n_pairs;
    dev.frame_bytes = frame_bytes, dev.valid_bytes = valid_bytes;
    dev.extra = (unsigned char *)(((uintptr_t)(d_valid + valid_bytes) + 15) & ~(uintptr_t)15);
    if ((rc = h2d(ctx, ctx->io[0], imgs, frame_bytes))) return rc;
    const unsigned char *d_gray = (const unsigned char *)ctx->io[0].p;
    if (n_pairs > 0) {
        if ((rc = canny_hip_dev_canny_corner_descriptors(ctx, d_gray, sigma, min_val, max_val, height, width, n_frames,
                                                         nullptr, mode, block, k_q8, quality_q16, min_response, min_dist,
                                                         corners_max, d_rec, d_cnt, nullptr, nullptr, nullptr, desc_options,
                                                         d_desc, d_meta)))
            return rc;
        if ((rc = canny_hip_dev_match_descriptors(ctx, d_desc, d_cnt, n_frames, corners_max, d_desc, d_cnt, n_frames,
                                                  corners_max, pairs.data(), n_pairs, max_distance, ratio_q8, match_options,
                                                  d_matches, d_pc)))
            return rc;
        if ((rc = canny_hip_dev_estimate_motion(ctx, d_rec, d_cnt, n_frames, corners_max, d_rec, d_cnt, n_frames,
                                                corners_max, pairs.data(), n_pairs, d_matches, model, thr_q4, hypotheses, seed,
                                                d_motion, nullptr)))
            return rc;
    }
    if ((rc = canny_hip_dev_compose_motion(ctx, n_pairs ? d_motion : nullptr, n_pairs, 0, d_xf))) return rc;
    return canny_hip_dev_warp_frames(ctx, d_gray, n_frames, height, width, d_xf, n_frames, height, width, interp, border,
                                     d_aligned, want_valid ? d_valid : nullptr);
}
} // namespace

int canny_hip_canny_align(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                          int height, int width, int mode, int block, int k_q8, int quality_q16, long long min_response,
                          int min_dist, int corners_max, int desc_options, int max_distance, int ratio_q8, int match_options,
                          int model, int thr_q4, int hypotheses, unsigned seed, int interp, int border,
                          unsigned char *aligned, long long *xforms, long long *motion, unsigned char *valid_bits)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!aligned) return CANNY_HIP_ERR_INVALID;
    AlignDev dev;
    if ((rc = align_on_device(ctx, imgs, n_frames, sigma, min_val, max_val, height, width, mode, block, k_q8, quality_q16,
                              min_response, min_dist, corners_max, desc_options, max_distance, ratio_q8, match_options, model,
                              thr_q4, hypotheses, seed, interp, border, xforms, motion, valid_bits != nullptr, 0, dev)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(aligned, dev.aligned, dev.frame_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(xforms, dev.xf, (size_t)n_frames * CANNY_HIP_XFORM_WORDS * sizeof(long long),
                                hipMemcpyDeviceToHost, ctx->stream));
    if (motion && dev.n_pairs)
        HIP_TRY(ctx, hipMemcpyAsync(motion, dev.motion, (size_t)dev.n_pairs * CANNY_HIP_MOTION_WORDS * sizeof(long long),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (valid_bits) HIP_TRY(ctx, hipMemcpyAsync(valid_bits, dev.valid, dev.valid_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_warp_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfWarp, CANNY_HIP_WARP_PARTS, part, total_ms, launches);
}

// Host-only: the launch plan of the warp and, for one record and tile, what the tiled route does with it.
int canny_hip_selftest_warp_plan(int n_out, int out_h, int out_w, unsigned long long *out, const long long *xform, int src_h,
                                 int src_w, int interp, int tile_x, int tile_y, int *box)
{
    if (!out || warp_check(1, 1, 1, n_out, out_h, out_w, 0, 0)) return CANNY_HIP_ERR_INVALID;
    const LaunchPlan p = plan_warp_tiles(n_out, out_h, out_w);
    store_plan(out, p);
    if (!xform) return CANNY_HIP_OK;
    if (!box || warp_check(1, src_h, src_w, 1, 1, 1, interp, 0) || tile_x < 0 || tile_y < 0 || tile_x * 64 >= out_w ||
        tile_y * 16 >= out_h)
        return CANNY_HIP_ERR_INVALID;
    box[0] = warp_tile_footprint(xform, interp, src_h, src_w, out_h, out_w, tile_x, tile_y, box + 1) ? 1 : 0;
    return CANNY_HIP_OK;
}

// ---- temporal fusion of aligned frames and change masks (canny_fuse.hip) ---------------------------
// canny_hip_fuse_frames and canny_hip_change_mask, the rules in plain C++, live in canny_fuse_host.cpp.

namespace {
// the stack both calls read
int fuse_stack_check(int n_frames, int h, int w)
{
    if (n_frames < 1 || h < 1 || w < 1) return CANNY_HIP_ERR_INVALID;
    if (h > 32768 || w > 32768 || (long long)h * w >= (1ll << 31) || n_frames > 65535) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// every check of the fusion but the pointers
int fuse_check(int n_frames, int h, int w, int group_len, int group_step, int op, int fill, int min_count)
{
    if (n_frames < 1 || h < 1 || w < 1 || group_len < 1 || group_len > CANNY_HIP_FUSE_MAX_GROUP || group_len > n_frames ||
        group_step < 1 || op < CANNY_HIP_FUSE_MEAN || op > CANNY_HIP_FUSE_MAX || fill < 0 || fill > 255 || min_count < 1 ||
        min_count > 255)
        return CANNY_HIP_ERR_INVALID;
    return fuse_stack_check(n_frames, h, w);
}

// ... and of the change mask
int mask_check(int n_frames, int h, int w, int frames_per_background, int thr, int min_count)
{
    if (n_frames < 1 || h < 1 || w < 1 || frames_per_background < 1 || thr < 0 || thr > 255 || min_count < 1 || min_count > 255)
        return CANNY_HIP_ERR_INVALID;
    return fuse_stack_check(n_frames, h, w);
}

bool opt_overlap(const void *a, size_t na, const void *b, size_t nb) { return a && b && ranges_overlap(a, na, b, nb); }
} // namespace

int canny_hip_dev_fuse_frames(canny_hip_ctx *ctx, const unsigned char *d_frames, const unsigned char *d_valid_bits,
                              int n_frames, int h, int w, int group_len, int group_step, int op, int fill, int min_count,
                              unsigned char *d_fused, unsigned char *d_count)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_frames || !d_fused) return CANNY_HIP_ERR_INVALID;
    if ((rc = fuse_check(n_frames, h, w, group_len, group_step, op, fill, min_count))) return rc;
    const int n_groups = (n_frames - group_len) / group_step + 1;
    const size_t in_bytes = npx(h, w, n_frames), vbytes = npx(h, (w + 7) / 8, n_frames), out_bytes = npx(h, w, n_groups);
    if (opt_overlap(d_frames, in_bytes, d_fused, out_bytes) || opt_overlap(d_frames, in_bytes, d_count, out_bytes) ||
        opt_overlap(d_valid_bits, vbytes, d_fused, out_bytes) || opt_overlap(d_valid_bits, vbytes, d_count, out_bytes) ||
        opt_overlap(d_fused, out_bytes, d_count, out_bytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    StageTimer tm(ctx, canny_hip_ctx::kProfFuse + CANNY_HIP_FUSE_PART_FUSE);
    HIP_TRY(ctx, launch_fuse_frames(d_frames, d_valid_bits, n_frames, h, w, group_len, group_step, op, fill, min_count,
                                    ctx->fuse_route, d_fused, d_count, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_dev_change_mask(canny_hip_ctx *ctx, const unsigned char *d_frames, const unsigned char *d_valid_bits,
                              int n_frames, int h, int w, const unsigned char *d_background,
                              const unsigned char *d_bg_count, int frames_per_background, int thr, int min_count,
                              unsigned char *d_mask_bits, long long *d_changed)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_frames || !d_background || !d_mask_bits || ((uintptr_t)d_changed & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = mask_check(n_frames, h, w, frames_per_background, thr, min_count))) return rc;
    const size_t n_bg = ((size_t)n_frames + frames_per_background - 1) / frames_per_background;
    const size_t in_bytes = npx(h, w, n_frames), vbytes = npx(h, (w + 7) / 8, n_frames), bg_bytes = (size_t)h * w * n_bg;
    const size_t ch_bytes = (size_t)n_frames * sizeof(long long);
    if (opt_overlap(d_frames, in_bytes, d_mask_bits, vbytes) || opt_overlap(d_valid_bits, vbytes, d_mask_bits, vbytes) ||
        opt_overlap(d_background, bg_bytes, d_mask_bits, vbytes) || opt_overlap(d_bg_count, bg_bytes, d_mask_bits, vbytes) ||
        opt_overlap(d_frames, in_bytes, d_changed, ch_bytes) || opt_overlap(d_valid_bits, vbytes, d_changed, ch_bytes) ||
        opt_overlap(d_background, bg_bytes, d_changed, ch_bytes) || opt_overlap(d_bg_count, bg_bytes, d_changed, ch_bytes) ||
        opt_overlap(d_mask_bits, vbytes, d_changed, ch_bytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    StageTimer tm(ctx, canny_hip_ctx::kProfFuse + CANNY_HIP_FUSE_PART_MASK);
    HIP_TRY(ctx, launch_change_mask(d_frames, d_valid_bits, n_frames, h, w, d_background, d_bg_count, frames_per_background,
                                    thr, min_count, d_mask_bits, (unsigned long long *)d_changed, ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_canny_background(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                               int max_val, int height, int width, int mode, int block, int k_q8, int quality_q16,
                               long long min_response, int min_dist, int corners_max, int desc_options, int max_distance,
                               int ratio_q8, int match_options, int model, int thr_q4, int hypotheses, unsigned seed,
                               int interp, int border, int op, int fill, int min_count, int thr, unsigned char *background,
                               unsigned char *count, unsigned char *mask_bits, long long *changed, long long *xforms)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!background || ((uintptr_t)changed & 7)) return CANNY_HIP_ERR_INVALID;
    // one window over the whole batch: group_len = n_frames
    if ((rc = fuse_check(n_frames, height, width, n_frames, n_frames, op, fill, min_count))) return rc;
    if ((rc = mask_check(n_frames, height, width, n_frames, thr, min_count))) return rc;
    const size_t plane = (size_t)height * width, mask_bytes = npx(height, (width + 7) / 8, n_frames);
    const size_t ch_bytes = (size_t)n_frames * sizeof(long long), plane16 = (plane + 15) & ~(size_t)15;
    AlignDev dev;
    // behind the valid bits: the counts of the frames | the fused plane | its counts | the masks
    if ((rc = align_on_device(ctx, imgs, n_frames, sigma, min_val, max_val, height, width, mode, block, k_q8, quality_q16,
                              min_response, min_dist, corners_max, desc_options, max_distance, ratio_q8, match_options, model,
                              thr_q4, hypotheses, seed, interp, border, xforms, nullptr, true,
                              ((ch_bytes + 15) & ~(size_t)15) + 2 * plane16 + mask_bytes, dev)))
        return rc;
    long long *d_changed = (long long *)dev.extra;
    unsigned char *d_bg = dev.extra + ((ch_bytes + 15) & ~(size_t)15), *d_cnt = d_bg + plane16, *d_mask = d_cnt + plane16;
    if ((rc = canny_hip_dev_fuse_frames(ctx, dev.aligned, dev.valid, n_frames, height, width, n_frames, n_frames, op, fill,
                                        min_count, d_bg, d_cnt)))
        return rc;
    if (mask_bits || changed) {
        if ((rc = canny_hip_dev_change_mask(ctx, dev.aligned, dev.valid, n_frames, height, width, d_bg, d_cnt, n_frames, thr,
                                            min_count, d_mask, changed ? d_changed : nullptr)))
            return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(background, d_bg, plane, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(xforms, dev.xf, (size_t)n_frames * CANNY_HIP_XFORM_WORDS * sizeof(long long),
                                hipMemcpyDeviceToHost, ctx->stream));
    if (count) HIP_TRY(ctx, hipMemcpyAsync(count, d_cnt, plane, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_bits) HIP_TRY(ctx, hipMemcpyAsync(mask_bits, d_mask, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (changed) HIP_TRY(ctx, hipMemcpyAsync(changed, d_changed, ch_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_fuse_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfFuse, CANNY_HIP_FUSE_PARTS, part, total_ms, launches);
}

// Host-only: the launch plans of the two capped launches of the temporal fusion.
int canny_hip_selftest_fuse_plan(int which, int n_frames, int h, int w, int group_len, int group_step, unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    LaunchPlan p;
    if (which == CANNY_HIP_FUSE_PART_FUSE) {
        if (fuse_check(n_frames, h, w, group_len, group_step, 0, 0, 1)) return CANNY_HIP_ERR_INVALID;
        p = plan_fuse_tiles((n_frames - group_len) / group_step + 1, h, w);
        p.aux = fuse_median_route(group_len, 0);
    } else if (which == CANNY_HIP_FUSE_PART_MASK) {
        if (fuse_stack_check(n_frames, h, w)) return CANNY_HIP_ERR_INVALID;
        p = plan_fuse_tiles(n_frames, h, w);
    } else {
        return CANNY_HIP_ERR_INVALID;
    }
    store_plan(out, p);
    return CANNY_HIP_OK;
}

int canny_hip_selftest_fuse_mean(canny_hip_ctx *ctx, unsigned char *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!out) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    const size_t bytes = (size_t)255 * CANNY_HIP_FUSE_MEAN_ROW;
    HIP_TRY(ctx, ctx->io[1].ensure(bytes));
    HIP_TRY(ctx, launch_fuse_mean_table((uint8_t *)ctx->io[1].p, ctx->stream));
    return d2h_sync(ctx, out, ctx->io[1].p, bytes);
}

// ---- binary morphology on packed bit maps (canny_morph.hip) -----------------------------------------
// canny_hip_morph_bits and canny_hip_morph_element, the rule in plain C++, live in canny_morph_host.cpp.

namespace {
// every check of the morphology but the pointers and the overlaps
int morph_check(int n_frames, int h, int w, int op, const unsigned *rows, int kw, int kh, int border, int iterations)
{
    if (n_frames < 1 || h < 1 || w < 1 || op < CANNY_HIP_MORPH_ERODE || op > CANNY_HIP_MORPH_BLACKHAT || !rows || kw < 1 ||
        kw > CANNY_HIP_MORPH_MAX_EXTENT || kh < 1 || kh > CANNY_HIP_MORPH_MAX_EXTENT || !(kw & 1) || !(kh & 1) ||
        border < CANNY_HIP_MORPH_BORDER_ZERO || border > CANNY_HIP_MORPH_BORDER_NEUTRAL || iterations < 1 ||
        iterations > CANNY_HIP_MORPH_MAX_ITERATIONS)
        return CANNY_HIP_ERR_INVALID;
    unsigned any = 0;
    for (int j = 0; j < kh; j++) {
        if (rows[j] >> kw) return CANNY_HIP_ERR_INVALID;
        any |= rows[j];
    }
    if (!any) return CANNY_HIP_ERR_INVALID;
    return fuse_stack_check(n_frames, h, w);
}

// The operator queued on the context's stream; src: a packed map or -- strong -- the context's strong bit-plane.  Everything
// has been checked.
int dev_morph(canny_hip_ctx *ctx, const void *src, bool strong, int n_frames, int h, int w, int op, const unsigned *rows,
              int kw, int kh, int border, int iterations, unsigned char *d_out, long long *d_counts)
{
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), slot = (bytes + 15) & ~(size_t)15;
    const int n_steps = (op <= CANNY_HIP_MORPH_DILATE ? 1 : 2) * iterations;
    uint8_t *ws_a = nullptr, *ws_b = nullptr;
    if (n_steps > 1) {
        HIP_TRY(ctx, ctx->morph_ws.ensure(2 * slot));
        ws_a = (uint8_t *)ctx->morph_ws.p, ws_b = ws_a + slot;
    }
    StageTimer tm(ctx, canny_hip_ctx::kProfMorph + CANNY_HIP_MORPH_PART_STEPS);
    HIP_TRY(ctx, launch_morph(src, strong, n_frames, h, w, op, rows, kw, kh, border, iterations, ctx->morph_route, ws_a, ws_b,
                              d_out, (unsigned long long *)d_counts, ctx->stream));
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_morph_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int h, int w, int op,
                             const unsigned *rows, int kw, int kh, int border, int iterations, unsigned char *d_out_bits,
                             long long *d_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_out_bits || ((uintptr_t)d_counts & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = morph_check(n_frames, h, w, op, rows, kw, kh, border, iterations))) return rc;
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), cbytes = (size_t)n_frames * sizeof(long long);
    if (ranges_overlap(d_bits, bytes, d_out_bits, bytes) || opt_overlap(d_bits, bytes, d_counts, cbytes) ||
        opt_overlap(d_out_bits, bytes, d_counts, cbytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_morph(ctx, d_bits, false, n_frames, h, w, op, rows, kw, kh, border, iterations, d_out_bits, d_counts);
}

int canny_hip_dev_canny_morph(canny_hip_ctx *ctx, int n_frames, int h, int w, int op, const unsigned *rows, int kw, int kh,
                              int border, int iterations, unsigned char *d_out_bits, long long *d_counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_out_bits || ((uintptr_t)d_counts & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = morph_check(n_frames, h, w, op, rows, kw, kh, border, iterations))) return rc;
    // the plane the last canny call left: only for the batch it belongs to
    if (!last_canny_was(ctx, n_frames, h, w) || !ctx->plane_s.p) return CANNY_HIP_ERR_INVALID;
    if (opt_overlap(d_out_bits, npx(h, (w + 7) / 8, n_frames), d_counts, (size_t)n_frames * sizeof(long long)))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_morph(ctx, ctx->plane_s.p, true, n_frames, h, w, op, rows, kw, kh, border, iterations, d_out_bits, d_counts);
}

int canny_hip_canny_morph(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                          int height, int width, int op, const unsigned *rows, int kw, int kh, int border, int iterations,
                          unsigned char *out_bits, long long *counts)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !out_bits || ((uintptr_t)counts & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = morph_check(n_frames, height, width, op, rows, kw, kh, border, iterations))) return rc;
    if ((rc = check_dims(height, width, n_frames))) return rc;
    const size_t n = npx(height, width, n_frames), bytes = npx(height, (width + 7) / 8, n_frames);
    const size_t cbytes = (size_t)n_frames * sizeof(long long), slot = (bytes + 15) & ~(size_t)15;
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: the output maps | the counts | the finished map as bits where the strong plane is not the map
    HIP_TRY(ctx, ctx->io[1].ensure(2 * slot + ((cbytes + 15) & ~(size_t)15)));
    unsigned char *d_out = (unsigned char *)ctx->io[1].p, *d_map = d_out + slot + ((cbytes + 15) & ~(size_t)15);
    long long *d_counts = (long long *)(d_out + slot);
    HIP_TRY(ctx, ctx->edges16.ensure(n * sizeof(short)));
    if ((rc = dev_canny(ctx, (const unsigned char *)ctx->io[0].p, sigma, min_val, max_val, height, width, n_frames,
                        (short *)ctx->edges16.p)))
        return rc;
    if (max_val > 255) { // the reference zeroes every reached pixel: the map, not the plane, is the source
        HIP_TRY(ctx, launch_edges_to_bits((const int16_t *)ctx->edges16.p, d_map, height, width, n_frames, ctx->stream));
        rc = dev_morph(ctx, d_map, false, n_frames, height, width, op, rows, kw, kh, border, iterations, d_out,
                       counts ? d_counts : nullptr);
    } else {
        rc = dev_morph(ctx, ctx->plane_s.p, true, n_frames, height, width, op, rows, kw, kh, border, iterations, d_out,
                       counts ? d_counts : nullptr);
    }
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_bits, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, cbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

int canny_hip_morph_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches)
{
    return profile_part_get(ctx, canny_hip_ctx::kProfMorph, CANNY_HIP_MORPH_PARTS, part, total_ms, launches);
}

// Host-only: the launch plan of one primitive step and the route automatic takes for a full rectangle of kw x kh.
int canny_hip_selftest_morph_plan(int n_frames, int h, int w, int kw, int kh, unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    if (kw < 1 || kw > CANNY_HIP_MORPH_MAX_EXTENT || kh < 1 || kh > CANNY_HIP_MORPH_MAX_EXTENT || !(kw & 1) || !(kh & 1))
        return CANNY_HIP_ERR_INVALID;
    const int rc = fuse_stack_check(n_frames, h, w);
    if (rc) return rc;
    const LaunchPlan p = plan_morph_tiles(n_frames, h, w);
    store_plan(out, p);
    out[4] = (unsigned long long)morph_auto_route(kw, kh); // the route, not aux
    return CANNY_HIP_OK;
}

// ---- binarization: gray planes to packed bit maps (canny_binarize.hip) ------------------------------
// canny_hip_binarize and canny_hip_otsu_from_histogram, the rule in plain C++, live in canny_binarize_host.cpp.

namespace {
constexpr long long kOtsuMaxPixels = 1ll << 26;

// every check of the binarization but the pointers and the overlaps
int binarize_check(int n_frames, int h, int w, int method, int thr_or_c, int kw, int kh, int invert)
{
    if (n_frames < 1 || h < 1 || w < 1 || invert < 0 || invert > 1) return CANNY_HIP_ERR_INVALID;
    if (method == CANNY_HIP_BIN_FIXED) {
        if (thr_or_c < -1 || thr_or_c > 255) return CANNY_HIP_ERR_INVALID;
    } else if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN) {
        if (thr_or_c < -255 || thr_or_c > 255 || kw < 3 || kw > CANNY_HIP_BIN_MAX_EXTENT || kh < 3 ||
            kh > CANNY_HIP_BIN_MAX_EXTENT || !(kw & 1) || !(kh & 1))
            return CANNY_HIP_ERR_INVALID;
    } else if (method != CANNY_HIP_BIN_OTSU) {
        return CANNY_HIP_ERR_INVALID;
    }
    const int rc = fuse_stack_check(n_frames, h, w);
    if (rc) return rc;
    if (method == CANNY_HIP_BIN_OTSU && (long long)h * w > kOtsuMaxPixels) return CANNY_HIP_ERR_UNSUPPORTED;
    return CANNY_HIP_OK;
}

// The operator queued on the context's stream; everything has been checked.
int dev_binarize(canny_hip_ctx *ctx, const void *plane, bool plane_u8, int n_frames, int h, int w, int method, int thr_or_c,
                 int kw, int kh, int invert, unsigned char *d_out, long long *d_counts, int *d_thresholds)
{
    // the workspace: the histograms (OTSU) | the thresholds where the caller has no buffer for them
    const size_t hist_bytes = method == CANNY_HIP_BIN_OTSU ? (((size_t)n_frames * kHistBins * sizeof(uint32_t) + 15) & ~(size_t)15) : 0;
    int *thr = d_thresholds;
    if (hist_bytes || (!thr && method != CANNY_HIP_BIN_ADAPTIVE_MEAN)) {
        HIP_TRY(ctx, ctx->binarize_ws.ensure(hist_bytes + (size_t)n_frames * sizeof(int)));
        if (!thr) thr = (int *)((unsigned char *)ctx->binarize_ws.p + hist_bytes);
    }
    if (method == CANNY_HIP_BIN_OTSU) {
        uint32_t *hist = (uint32_t *)ctx->binarize_ws.p;
        {
            StageTimer tm(ctx, canny_hip_ctx::kProfBinarize + CANNY_HIP_BIN_PART_HISTOGRAM);
            HIP_TRY(ctx, hipMemsetAsync(hist, 0, (size_t)n_frames * kHistBins * sizeof(uint32_t), ctx->stream));
            HIP_TRY(ctx, launch_hist_intensity(plane, plane_u8, hist, h, w, n_frames, ctx->stream));
        }
        StageTimer tm(ctx, canny_hip_ctx::kProfBinarize + CANNY_HIP_BIN_PART_SELECT);
        HIP_TRY(ctx, launch_binarize_otsu(hist, n_frames, thr, ctx->stream));
    }
    StageTimer tm(ctx, canny_hip_ctx::kProfBinarize + CANNY_HIP_BIN_PART_MAP);
    if (method != CANNY_HIP_BIN_OTSU && thr) // FIXED: the kernel's thresholds; ADAPTIVE_MEAN: only what the caller reads
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)thr, thr_or_c, (size_t)n_frames, ctx->stream));
    if (method == CANNY_HIP_BIN_ADAPTIVE_MEAN)
        HIP_TRY(ctx, launch_binarize_adaptive(plane, plane_u8, n_frames, h, w, thr_or_c, kw, kh, invert, ctx->binarize_route,
                                              d_out, (unsigned long long *)d_counts, ctx->stream));
    else
        HIP_TRY(ctx, launch_binarize_map(plane, plane_u8, n_frames, h, w, thr, invert, d_out, (unsigned long long *)d_counts,
                                         ctx->stream));
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_binarize(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int method,
                           int thr_or_c, int kw, int kh, int invert, unsigned char *d_out_bits, long long *d_counts,
                           int *d_thresholds)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_out_bits || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_thresholds & 3)) return CANNY_HIP_ERR_INVALID;
    if ((rc = binarize_check(n_frames, h, w, method, thr_or_c, kw, kh, invert))) return rc;
    const void *plane = d_plane;
    bool plane_u8 = true;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, h, w) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        plane = ctx->smoothed.p;
        plane_u8 = ctx->last_canny_u8 != 0;
    }
    const size_t in_bytes = npx(h, w, n_frames) * (plane_u8 ? 1 : 2), bytes = npx(h, (w + 7) / 8, n_frames);
    const size_t cbytes = (size_t)n_frames * sizeof(long long), tbytes = (size_t)n_frames * sizeof(int);
    if (ranges_overlap(plane, in_bytes, d_out_bits, bytes) || opt_overlap(plane, in_bytes, d_counts, cbytes) ||
        opt_overlap(plane, in_bytes, d_thresholds, tbytes) || opt_overlap(d_out_bits, bytes, d_counts, cbytes) ||
        opt_overlap(d_out_bits, bytes, d_thresholds, tbytes) || opt_overlap(d_counts, cbytes, d_thresholds, tbytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_binarize(ctx, plane, plane_u8, n_frames, h, w, method, thr_or_c, kw, kh, invert, d_out_bits, d_counts,
                        d_thresholds);
}

int canny_hip_binarize_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int method,
                             int thr_or_c, int kw, int kh, int invert, unsigned char *out_bits, long long *counts,
                             int *thresholds)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !out_bits || ((uintptr_t)counts & 7) || ((uintptr_t)thresholds & 3)) return CANNY_HIP_ERR_INVALID;
    if ((rc = binarize_check(n_frames, h, w, method, thr_or_c, kw, kh, invert))) return rc;
    const size_t n = npx(h, w, n_frames), bytes = npx(h, (w + 7) / 8, n_frames), slot = (bytes + 15) & ~(size_t)15;
    const size_t cbytes = (size_t)n_frames * sizeof(long long), tbytes = (size_t)n_frames * sizeof(int);
    if (ranges_overlap(imgs, n, out_bits, bytes) || opt_overlap(imgs, n, counts, cbytes) ||
        opt_overlap(imgs, n, thresholds, tbytes) || opt_overlap(out_bits, bytes, counts, cbytes) ||
        opt_overlap(out_bits, bytes, thresholds, tbytes) || opt_overlap(counts, cbytes, thresholds, tbytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], imgs, n))) return rc;
    // one staging block: the output maps | the counts | the thresholds
    HIP_TRY(ctx, ctx->io[1].ensure(slot + ((cbytes + 15) & ~(size_t)15) + tbytes));
    unsigned char *d_out = (unsigned char *)ctx->io[1].p;
    long long *d_counts = (long long *)(d_out + slot);
    int *d_thr = (int *)(d_out + slot + ((cbytes + 15) & ~(size_t)15));
    if ((rc = dev_binarize(ctx, ctx->io[0].p, true, n_frames, h, w, method, thr_or_c, kw, kh, invert, d_out,
                           counts ? d_counts : nullptr, thresholds ? d_thr : nullptr)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_bits, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, cbytes, hipMemcpyDeviceToHost, ctx->stream));
    if (thresholds) HIP_TRY(ctx, hipMemcpyAsync(thresholds, d_thr, tbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

// Every group of kProfGroups by name: what the named getters answer, for this and later features.
int canny_hip_profile_part_get(canny_hip_ctx *ctx, const char *feature, int part, double *total_ms, long *launches)
{
    if (!feature) return CANNY_HIP_ERR_INVALID;
    int base = 0;
    for (const ProfGroup &g : kProfGroups) {
        if (!std::strcmp(feature, g.name)) return profile_part_get(ctx, base, g.parts, part, total_ms, launches);
        base += g.parts;
    }
    return CANNY_HIP_ERR_INVALID;
}

// Host-only: the launch plan of the kernel that writes the bits, and what the tests need to know about the marching tiling.
int canny_hip_selftest_binarize_plan(int n_frames, int h, int w, int method, int kw, int kh, unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    const bool adaptive = method == CANNY_HIP_BIN_ADAPTIVE_MEAN;
    if (!adaptive) kw = kh = 3; // ignored, like the calls ignore them
    const int rc = binarize_check(n_frames, h, w, method, 0, kw, kh, 0);
    if (rc) return rc;
    const int route = adaptive ? binarize_auto_route(kw, kh) : 0;
    const LaunchPlan bytes = plan_binarize_bytes(n_frames, h, w), march = plan_binarize_march(n_frames, h, w, kh);
    store_plan(out, route == 2 ? march : bytes);
    out[4] = (unsigned long long)route; // the route, not aux
    out[5] = (unsigned long long)binarize_strip_cols();
    out[6] = (unsigned long long)binarize_segment_rows(kh);
    out[7] = bytes.trips();
    out[8] = march.trips();
    out[9] = (unsigned long long)binarize_staged_cols(kw);
    return CANNY_HIP_OK;
}

// ---- thinning of packed bit maps (canny_thin.hip) ---------------------------------------------------
// canny_hip_thin_bits, the rule in plain C++, lives in canny_thin_host.cpp.

namespace {
// every check of the thinning but the pointers and the overlaps
int thin_check(int n_frames, int h, int w, int method, int max_iterations)
{
    if (n_frames < 1 || h < 1 || w < 1 || method < CANNY_HIP_THIN_ZHANGSUEN || method > CANNY_HIP_THIN_GUOHALL ||
        max_iterations < 0 || max_iterations > CANNY_HIP_THIN_MAX_ITERATIONS)
        return CANNY_HIP_ERR_INVALID;
    return fuse_stack_check(n_frames, h, w);
}

// The operator on the context's stream; src: a packed map or -- strong -- the context's strong bit-plane.  Everything has been
// checked.  max_iterations >= 1: queued; 0: the stream is idle when this returns.
int dev_thin(canny_hip_ctx *ctx, const void *src, bool strong, int n_frames, int h, int w, int method, int max_iterations,
             unsigned char *d_out, long long *d_info)
{
    HIP_TRY(ctx, ctx->thin_ws.ensure(thin_workspace_bytes(n_frames, h, w)));
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfThin + CANNY_HIP_THIN_PART_INFO);
        HIP_TRY(ctx, launch_thin_zero(ctx->thin_ws.p, n_frames, h, w, d_info, ctx->stream));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfThin + CANNY_HIP_THIN_PART_PASSES);
        HIP_TRY(ctx, launch_thin_passes(src, strong, n_frames, h, w, method, max_iterations, ctx->thin_route, ctx->thin_fuse,
                                        ctx->thin_ws.p, d_out, ctx->stream));
    }
    if (d_info) {
        StageTimer tm(ctx, canny_hip_ctx::kProfThin + CANNY_HIP_THIN_PART_INFO);
        HIP_TRY(ctx, launch_thin_info(ctx->thin_ws.p, n_frames, h, w, max_iterations, d_info, ctx->stream));
    }
    if (!max_iterations) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // as documented: also behind the last launches
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_thin_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int h, int w, int method,
                            int max_iterations, unsigned char *d_out_bits, long long *d_info)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_bits || !d_out_bits || ((uintptr_t)d_info & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = thin_check(n_frames, h, w, method, max_iterations))) return rc;
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), ibytes = (size_t)n_frames * CANNY_HIP_THIN_INFO * sizeof(long long);
    if (ranges_overlap(d_bits, bytes, d_out_bits, bytes) || opt_overlap(d_bits, bytes, d_info, ibytes) ||
        opt_overlap(d_out_bits, bytes, d_info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_thin(ctx, d_bits, false, n_frames, h, w, method, max_iterations, d_out_bits, d_info);
}

int canny_hip_dev_canny_thin(canny_hip_ctx *ctx, int n_frames, int h, int w, int method, int max_iterations,
                             unsigned char *d_out_bits, long long *d_info)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_out_bits || ((uintptr_t)d_info & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = thin_check(n_frames, h, w, method, max_iterations))) return rc;
    // the plane the last canny call left: only for the batch it belongs to
    if (!last_canny_was(ctx, n_frames, h, w) || !ctx->plane_s.p) return CANNY_HIP_ERR_INVALID;
    if (opt_overlap(d_out_bits, npx(h, (w + 7) / 8, n_frames), d_info, (size_t)n_frames * CANNY_HIP_THIN_INFO * sizeof(long long)))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_thin(ctx, ctx->plane_s.p, true, n_frames, h, w, method, max_iterations, d_out_bits, d_info);
}

int canny_hip_thin_batch(canny_hip_ctx *ctx, const unsigned char *bits, int n_frames, int h, int w, int method,
                         int max_iterations, unsigned char *out_bits, long long *info)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!bits || !out_bits || ((uintptr_t)info & 7)) return CANNY_HIP_ERR_INVALID;
    if ((rc = thin_check(n_frames, h, w, method, max_iterations))) return rc;
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), slot = (bytes + 15) & ~(size_t)15;
    const size_t ibytes = (size_t)n_frames * CANNY_HIP_THIN_INFO * sizeof(long long);
    if (ranges_overlap(bits, bytes, out_bits, bytes) || opt_overlap(bits, bytes, info, ibytes) ||
        opt_overlap(out_bits, bytes, info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], bits, bytes))) return rc;
    // one staging block: the output maps | the info
    HIP_TRY(ctx, ctx->io[1].ensure(slot + ibytes));
    unsigned char *d_out = (unsigned char *)ctx->io[1].p;
    long long *d_info = (long long *)(d_out + slot);
    if ((rc = dev_thin(ctx, ctx->io[0].p, false, n_frames, h, w, method, max_iterations, d_out, info ? d_info : nullptr)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_bits, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (info) HIP_TRY(ctx, hipMemcpyAsync(info, d_info, ibytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

// Host-only: the launch plan of every launch of a call and the full iterations a launch runs.
int canny_hip_selftest_thin_plan(int n_frames, int h, int w, int fuse, unsigned long long *out)
{
    if (!out || fuse < 0 || fuse > 8) return CANNY_HIP_ERR_INVALID;
    const int rc = fuse_stack_check(n_frames, h, w);
    if (rc) return rc;
    store_plan(out, plan_thin_tiles(n_frames, h, w));
    out[4] = (unsigned long long)(fuse ? fuse : thin_auto_fuse()); // aux: the full iterations a launch runs
    return CANNY_HIP_OK;
}

// ---- grey-level morphology and median filtering of u8 planes (canny_gray_morph.hip) ------------------
// canny_hip_gray_morph, the rule in plain C++, lives in canny_gray_morph_host.cpp.

namespace {
// every check of the grey-level morphology but the pointers and the overlaps
int gray_morph_check(int n_frames, int h, int w, int op, const unsigned *rows, int kw, int kh, int border_mode, int border_value,
                     int iterations)
{
    if (op < CANNY_HIP_GRAY_ERODE || op > CANNY_HIP_GRAY_MEDIAN || border_mode < CANNY_HIP_GRAY_BORDER_NEUTRAL ||
        border_mode > CANNY_HIP_GRAY_BORDER_CONSTANT ||
        (border_mode == CANNY_HIP_GRAY_BORDER_CONSTANT && (border_value < 0 || border_value > 255)))
        return CANNY_HIP_ERR_INVALID;
    // the element, the iterations and the limits: the binary morphology's own checks
    const int rc = morph_check(n_frames, h, w, CANNY_HIP_MORPH_ERODE, rows, kw, kh, CANNY_HIP_MORPH_BORDER_NEUTRAL, iterations);
    if (rc == CANNY_HIP_ERR_INVALID) return rc;
    if (op == CANNY_HIP_GRAY_MEDIAN) {
        if (kw != kh || (kw != 3 && kw != 5) || border_mode == CANNY_HIP_GRAY_BORDER_NEUTRAL) return CANNY_HIP_ERR_INVALID;
        for (int j = 0; j < kh; j++)
            if (rows[j] != (1u << kw) - 1u) return CANNY_HIP_ERR_INVALID;
    }
    return rc;
}

// The operator queued on the context's stream; everything has been checked.
int dev_gray_morph(canny_hip_ctx *ctx, const void *plane, bool plane_u8, int n_frames, int h, int w, int op, const unsigned *rows,
                   int kw, int kh, int border_mode, int border_value, int iterations, unsigned char *d_out)
{
    const size_t bytes = npx(h, w, n_frames), slot = (bytes + 15) & ~(size_t)15;
    const bool single = op <= CANNY_HIP_GRAY_DILATE || op == CANNY_HIP_GRAY_MEDIAN;
    const int n_steps = (single ? 1 : 2) * iterations;
    uint8_t *ws_a = nullptr, *ws_b = nullptr;
    if (n_steps > 1) {
        HIP_TRY(ctx, ctx->morph_ws.ensure(2 * slot)); // shared with the binary morphology: no call reads what another left
        ws_a = (uint8_t *)ctx->morph_ws.p, ws_b = ws_a + slot;
    }
    StageTimer tm(ctx, canny_hip_ctx::kProfGrayMorph + CANNY_HIP_GRAY_PART_STEPS);
    HIP_TRY(ctx, launch_gray_morph(plane, !plane_u8, n_frames, h, w, op, rows, kw, kh, border_mode, border_value, iterations,
                                   ctx->gray_morph_route, ws_a, ws_b, d_out, ctx->stream));
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_gray_morph(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int op,
                             const unsigned *rows, int kw, int kh, int border_mode, int border_value, int iterations,
                             unsigned char *d_out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_out) return CANNY_HIP_ERR_INVALID;
    if ((rc = gray_morph_check(n_frames, h, w, op, rows, kw, kh, border_mode, border_value, iterations))) return rc;
    const void *plane = d_plane;
    bool plane_u8 = true;
    if (!d_plane) {
        // the plane the last canny call left: only for the batch it belongs to
        if (!last_canny_was(ctx, n_frames, h, w) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
        plane = ctx->smoothed.p;
        plane_u8 = ctx->last_canny_u8 != 0;
    }
    const size_t bytes = npx(h, w, n_frames);
    if (ranges_overlap(plane, bytes * (plane_u8 ? 1 : 2), d_out, bytes)) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_gray_morph(ctx, plane, plane_u8, n_frames, h, w, op, rows, kw, kh, border_mode, border_value, iterations, d_out);
}

int canny_hip_gray_morph_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int op,
                               const unsigned *rows, int kw, int kh, int border_mode, int border_value, int iterations,
                               unsigned char *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !out) return CANNY_HIP_ERR_INVALID;
    if ((rc = gray_morph_check(n_frames, h, w, op, rows, kw, kh, border_mode, border_value, iterations))) return rc;
    const size_t bytes = npx(h, w, n_frames);
    if (ranges_overlap(imgs, bytes, out, bytes)) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], imgs, bytes))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(bytes));
    if ((rc = dev_gray_morph(ctx, ctx->io[0].p, true, n_frames, h, w, op, rows, kw, kh, border_mode, border_value, iterations,
                             (unsigned char *)ctx->io[1].p)))
        return rc;
    return d2h_sync(ctx, out, ctx->io[1].p, bytes);
}

// Host-only: the launch plan of one primitive step and the route automatic takes for op with a full rectangle of kw x kh.
int canny_hip_selftest_gray_morph_plan(int n_frames, int h, int w, int op, int kw, int kh, unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    if (op < CANNY_HIP_GRAY_ERODE || op > CANNY_HIP_GRAY_MEDIAN || kw < 1 || kw > CANNY_HIP_MORPH_MAX_EXTENT || kh < 1 ||
        kh > CANNY_HIP_MORPH_MAX_EXTENT || !(kw & 1) || !(kh & 1) ||
        (op == CANNY_HIP_GRAY_MEDIAN && (kw != kh || (kw != 3 && kw != 5))))
        return CANNY_HIP_ERR_INVALID;
    const int rc = fuse_stack_check(n_frames, h, w);
    if (rc) return rc;
    store_plan(out, plan_gray_morph_tiles(n_frames, h, w));
    out[4] = (unsigned long long)gray_morph_auto_route(op, kw, kh); // the route, not aux
    return CANNY_HIP_OK;
}

// ---- image pyramids of u8 planes (canny_pyramid.hip) ------------------------------------------------
// canny_hip_pyramid_layout, canny_hip_pyramid and canny_hip_pyr_up, the rule in plain C++, live in canny_pyramid_host.cpp.

namespace {
// The plane a pyrDown reads: the caller's, or for NULL the smoothed plane the last canny call of this geometry left.
int pyr_source(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, const void **plane, bool *plane_u8)
{
    *plane = d_plane, *plane_u8 = true;
    if (d_plane) return CANNY_HIP_OK;
    if (!last_canny_was(ctx, n_frames, h, w) || !ctx->smoothed.p) return CANNY_HIP_ERR_INVALID;
    *plane = ctx->smoothed.p, *plane_u8 = ctx->last_canny_u8 != 0;
    return CANNY_HIP_OK;
}

// The levels queued on the context's stream, one launch each; everything has been checked.  info: the layout.
int dev_pyramid(canny_hip_ctx *ctx, const void *plane, bool plane_u8, int n_frames, int h, int w, int levels, const long long *info,
                unsigned char *d_out)
{
    StageTimer tm(ctx, canny_hip_ctx::kProfPyramid + CANNY_HIP_PYR_PART_DOWN);
    for (int l = 0; l < levels; l++) {
        unsigned char *level = d_out + info[4 * l + 2];
        HIP_TRY(ctx, launch_pyr_down(plane, !plane_u8, n_frames, h, w, ctx->pyramid_route, level, ctx->stream));
        plane = level, plane_u8 = true, h = (int)info[4 * l], w = (int)info[4 * l + 1];
    }
    return CANNY_HIP_OK;
}

// every check of pyrUp but the pointers and the overlap
int pyr_up_check(int n_frames, int h, int w, int oh, int ow)
{
    if (n_frames < 1 || h < 1 || w < 1 || (oh != 2 * h - 1 && oh != 2 * h) || (ow != 2 * w - 1 && ow != 2 * w) || oh < 1 || ow < 1)
        return CANNY_HIP_ERR_INVALID;
    const int rc = fuse_stack_check(n_frames, h, w);
    return rc ? rc : fuse_stack_check(n_frames, oh, ow);
}

int dev_pyr_up(canny_hip_ctx *ctx, const unsigned char *plane, int n_frames, int h, int w, int oh, int ow, unsigned char *d_out)
{
    StageTimer tm(ctx, canny_hip_ctx::kProfPyramid + CANNY_HIP_PYR_PART_UP);
    HIP_TRY(ctx, launch_pyr_up(plane, n_frames, h, w, oh, ow, d_out, ctx->stream));
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_pyr_down(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, unsigned char *d_out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_out) return CANNY_HIP_ERR_INVALID;
    if ((rc = fuse_stack_check(n_frames, h, w))) return rc;
    const void *plane;
    bool plane_u8;
    if ((rc = pyr_source(ctx, d_plane, n_frames, h, w, &plane, &plane_u8))) return rc;
    const long long level[4] = {(h + 1) / 2, (w + 1) / 2, 0, 0};
    if (ranges_overlap(plane, npx(h, w, n_frames) * (plane_u8 ? 1 : 2), d_out, npx((int)level[0], (int)level[1], n_frames)))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_pyramid(ctx, plane, plane_u8, n_frames, h, w, 1, level, d_out);
}

int canny_hip_dev_pyramid(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int levels,
                          unsigned char *d_out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_out) return CANNY_HIP_ERR_INVALID;
    long long info[4 * CANNY_HIP_PYR_MAX_LEVELS], total = 0;
    if ((rc = canny_hip_pyramid_layout(n_frames, h, w, levels, info, &total))) return rc;
    const void *plane;
    bool plane_u8;
    if ((rc = pyr_source(ctx, d_plane, n_frames, h, w, &plane, &plane_u8))) return rc;
    if (ranges_overlap(plane, npx(h, w, n_frames) * (plane_u8 ? 1 : 2), d_out, (size_t)total)) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_pyramid(ctx, plane, plane_u8, n_frames, h, w, levels, info, d_out);
}

int canny_hip_dev_pyr_up(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int oh, int ow,
                         unsigned char *d_out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_plane || !d_out) return CANNY_HIP_ERR_INVALID;
    if ((rc = pyr_up_check(n_frames, h, w, oh, ow))) return rc;
    if (ranges_overlap(d_plane, npx(h, w, n_frames), d_out, npx(oh, ow, n_frames))) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_pyr_up(ctx, d_plane, n_frames, h, w, oh, ow, d_out);
}

int canny_hip_pyramid_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int levels,
                            unsigned char *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !out) return CANNY_HIP_ERR_INVALID;
    long long info[4 * CANNY_HIP_PYR_MAX_LEVELS], total = 0;
    if ((rc = canny_hip_pyramid_layout(n_frames, h, w, levels, info, &total))) return rc;
    const size_t bytes = npx(h, w, n_frames);
    if (ranges_overlap(imgs, bytes, out, (size_t)total)) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], imgs, bytes))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure((size_t)total));
    unsigned char *d_out = (unsigned char *)ctx->io[1].p;
    if ((rc = dev_pyramid(ctx, ctx->io[0].p, true, n_frames, h, w, levels, info, d_out))) return rc;
    // level by level: the pad bytes of the caller's buffer stay as they are
    for (int l = 0; l + 1 < levels; l++)
        HIP_TRY(ctx, hipMemcpyAsync(out + info[4 * l + 2], d_out + info[4 * l + 2], (size_t)info[4 * l + 3], hipMemcpyDeviceToHost,
                                    ctx->stream));
    const long long *last = info + 4 * (levels - 1);
    return d2h_sync(ctx, out + last[2], d_out + last[2], (size_t)last[3]);
}

int canny_hip_pyr_up_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int oh, int ow,
                           unsigned char *out)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!imgs || !out) return CANNY_HIP_ERR_INVALID;
    if ((rc = pyr_up_check(n_frames, h, w, oh, ow))) return rc;
    const size_t bytes = npx(h, w, n_frames), out_bytes = npx(oh, ow, n_frames);
    if (ranges_overlap(imgs, bytes, out, out_bytes)) return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], imgs, bytes))) return rc;
    HIP_TRY(ctx, ctx->io[1].ensure(out_bytes));
    if ((rc = dev_pyr_up(ctx, (const unsigned char *)ctx->io[0].p, n_frames, h, w, oh, ow, (unsigned char *)ctx->io[1].p))) return rc;
    return d2h_sync(ctx, out, ctx->io[1].p, out_bytes);
}

// Host-only: the launch plan of one pyrDown of planes [n_frames][h][w] and the route automatic takes.
int canny_hip_selftest_pyramid_plan(int n_frames, int h, int w, unsigned long long *out)
{
    if (!out) return CANNY_HIP_ERR_INVALID;
    const int rc = fuse_stack_check(n_frames, h, w);
    if (rc) return rc;
    store_plan(out, plan_pyramid_tiles(n_frames, (h + 1) / 2, (w + 1) / 2));
    out[4] = (unsigned long long)pyramid_auto_route(); // the route, not aux
    return CANNY_HIP_OK;
}

// ---- morphological reconstruction of packed bit maps (canny_reconstruct.hip) ------------------------
// canny_hip_reconstruct_bits, the rule in plain C++, lives in canny_reconstruct_host.cpp.

namespace {
// every check of the reconstruction but the mask pointer and the overlaps
int recon_check(const void *marker, const void *out, const void *info, int n_frames, int h, int w, int op, int connectivity)
{
    if (!out || ((uintptr_t)info & 7) || n_frames < 1 || h < 1 || w < 1 || op < CANNY_HIP_RECON_SEEDED ||
        op > CANNY_HIP_RECON_CLEAR_BORDER || (connectivity != 4 && connectivity != 8) ||
        (op == CANNY_HIP_RECON_SEEDED) != (marker != nullptr))
        return CANNY_HIP_ERR_INVALID;
    return fuse_stack_check(n_frames, h, w);
}

// The operator on the context's stream; mask: a packed map or -- strong -- the context's strong bit-plane.  Everything has
// been checked.  The stream is idle when this returns.
int dev_reconstruct(canny_hip_ctx *ctx, const unsigned char *marker, const void *mask, bool strong, int n_frames, int h, int w,
                    int op, int connectivity, unsigned char *d_out, long long *d_info)
{
    HIP_TRY(ctx, ctx->thin_ws.ensure(reconstruct_workspace_bytes(n_frames, h, w)));
    auto phase = [&](int which) {
        return launch_reconstruct(which, marker, mask, strong, n_frames, h, w, op, connectivity, ctx->reconstruct_route,
                                  ctx->thin_ws.p, d_out, d_info, &ctx->last_reconstruct_launches, ctx->stream);
    };
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfReconstruct + CANNY_HIP_RECON_PART_INFO);
        HIP_TRY(ctx, phase(RECON_INIT));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfReconstruct + CANNY_HIP_RECON_PART_SWEEPS);
        HIP_TRY(ctx, phase(RECON_SWEEPS));
    }
    {
        StageTimer tm(ctx, canny_hip_ctx::kProfReconstruct + CANNY_HIP_RECON_PART_INFO);
        HIP_TRY(ctx, phase(RECON_FINISH));
    }
    return CANNY_HIP_OK;
}
} // namespace

int canny_hip_dev_reconstruct_bits(canny_hip_ctx *ctx, const unsigned char *d_marker, const unsigned char *d_mask, int n_frames,
                                   int h, int w, int op, int connectivity, unsigned char *d_out, long long *d_info)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!d_mask) return CANNY_HIP_ERR_INVALID;
    if ((rc = recon_check(d_marker, d_out, d_info, n_frames, h, w, op, connectivity))) return rc;
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), ibytes = (size_t)n_frames * CANNY_HIP_RECON_INFO * sizeof(long long);
    if (opt_overlap(d_marker, bytes, d_out, bytes) || ranges_overlap(d_mask, bytes, d_out, bytes) ||
        opt_overlap(d_out, bytes, d_info, ibytes) || opt_overlap(d_marker, bytes, d_info, ibytes) ||
        opt_overlap(d_mask, bytes, d_info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_reconstruct(ctx, d_marker, d_mask, false, n_frames, h, w, op, connectivity, d_out, d_info);
}

int canny_hip_dev_canny_reconstruct(canny_hip_ctx *ctx, const unsigned char *d_marker, int n_frames, int h, int w, int op,
                                    int connectivity, unsigned char *d_out, long long *d_info)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if ((rc = recon_check(d_marker, d_out, d_info, n_frames, h, w, op, connectivity))) return rc;
    // the plane the last canny call left: only for the batch it belongs to
    if (!last_canny_was(ctx, n_frames, h, w) || !ctx->plane_s.p) return CANNY_HIP_ERR_INVALID;
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), ibytes = (size_t)n_frames * CANNY_HIP_RECON_INFO * sizeof(long long);
    if (opt_overlap(d_marker, bytes, d_out, bytes) || opt_overlap(d_out, bytes, d_info, ibytes) ||
        opt_overlap(d_marker, bytes, d_info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    return dev_reconstruct(ctx, d_marker, ctx->plane_s.p, true, n_frames, h, w, op, connectivity, d_out, d_info);
}

int canny_hip_reconstruct_batch(canny_hip_ctx *ctx, const unsigned char *marker, const unsigned char *mask, int n_frames, int h,
                                int w, int op, int connectivity, unsigned char *out, long long *info)
{
    int rc = bind(ctx);
    if (rc) return rc;
    if (!mask) return CANNY_HIP_ERR_INVALID;
    if ((rc = recon_check(marker, out, info, n_frames, h, w, op, connectivity))) return rc;
    const size_t bytes = npx(h, (w + 7) / 8, n_frames), slot = (bytes + 15) & ~(size_t)15;
    const size_t ibytes = (size_t)n_frames * CANNY_HIP_RECON_INFO * sizeof(long long);
    if (opt_overlap(marker, bytes, out, bytes) || ranges_overlap(mask, bytes, out, bytes) || opt_overlap(out, bytes, info, ibytes) ||
        opt_overlap(marker, bytes, info, ibytes) || opt_overlap(mask, bytes, info, ibytes))
        return CANNY_HIP_ERR_INVALID;
    if ((rc = finish_pending(ctx))) return rc;
    if ((rc = h2d(ctx, ctx->io[0], mask, bytes))) return rc;
    if (marker && (rc = h2d(ctx, ctx->io[2], marker, bytes))) return rc;
    // one staging block: the output maps | the info
    HIP_TRY(ctx, ctx->io[1].ensure(slot + ibytes));
    unsigned char *d_out = (unsigned char *)ctx->io[1].p;
    long long *d_info = (long long *)(d_out + slot);
    if ((rc = dev_reconstruct(ctx, marker ? (const unsigned char *)ctx->io[2].p : nullptr, ctx->io[0].p, false, n_frames, h, w, op,
                              connectivity, d_out, info ? d_info : nullptr)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (info) HIP_TRY(ctx, hipMemcpyAsync(info, d_info, ibytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CANNY_HIP_OK;
}

// Host-only: the launch plan of the sweep launches of a call and the route automatic takes.
int canny_hip_selftest_reconstruct_plan(int n_frames, int h, int w, int route, unsigned long long *out)
{
    if (!out || route < 0 || route > 2) return CANNY_HIP_ERR_INVALID;
    const int rc = fuse_stack_check(n_frames, h, w);
    if (rc) return rc;
    store_plan(out, plan_reconstruct(n_frames, h, w, route));
    out[4] = (unsigned long long)reconstruct_auto_route(); // aux: the route automatic takes
    return CANNY_HIP_OK;
}

} // extern "C"
