/*
 * canny_hip.h -- C ABI of libcanny_hip.so: the MI355X (gfx950) Canny hot path.
 *
 * This is the drop-in boundary for StevenChang5/Canny_Edge's stage functions.  Every entry point
 * takes plain pointers and sizes (no C++ references, no torch types) so that it can be bound from
 * C, C++ (include/utils.h shims), Python ctypes (canny_edge_amd/capi.py) or any other FFI.
 *
 * Reference interface each function replaces (paths relative to the reference checkout):
 *
 *   canny_hip_gaussian_kernel      createGaussianKernel     src/utils.h:10   src/utils.cpp:77-95
 *   canny_hip_gaussian             gaussian                 src/utils.h:8    src/utils.cpp:26-68
 *                                  cuda_gaussian            src/cuda.h:4     src/cuda.cu:75-102
 *   canny_hip_xy_gradient          calculateXYGradient      src/utils.h:12   src/utils.cpp:106-187
 *   canny_hip_sobel                sobelOperator            src/utils.h:14   src/utils.cpp:201-236
 *                                  cuda_sobel               src/cuda.h:6     src/cuda.cu:220-246
 *   canny_hip_nms                  nonmaximalSuppression    src/utils.h:16   src/utils.cpp:248-308
 *                                  cuda_nonmaixmal_suppression src/cuda.h:8  src/cuda.cu:366-390
 *   canny_hip_hysteresis           hysteresis               src/utils.h:18   src/utils.cpp:322-342
 *   canny_hip_find_edge_pixels     findEdgePixels           src/utils.h:20   src/utils.cpp:360-427
 *   canny_hip_canny                canny / cuda_canny       src/utils.h:22   src/utils.cpp:429-492
 *                                                           src/cuda.h:10    src/cuda.cu:392-450
 *
 * Conventions (same as the reference): images are dense row-major, pixel (r,c) at r*width+c;
 * argument order is (..., height, width, ...); `short` planes are int16; thresholds are ints.
 * Unlike the reference's void functions every call returns a status (0 = CANNY_HIP_OK).
 * Results are bit-identical to the reference's CPU path (src/utils.cpp) on the documented domain.
 *
 * Numeric domain:
 *   - gaussian: any u8 image, sigma finite and > 0, window 1+2*ceil(3*sigma) <= CANNY_HIP_MAX_WINDOW.
 *   - xy_gradient / sobel / sobel_nms: height >= 2 and width >= 2 (the reference reads out of bounds
 *     below that).  Gradients are stored through short exactly like the reference.  Angle bins are
 *     computed with an exact integer rule that is proven equal to the reference's
 *     atan2/float expression for every |gx|,|gy| <= 1020, i.e. for every smoothed plane in [0,255]
 *     (everything gaussian() can produce); outside that range a gradient lying within float rounding
 *     of a bin boundary may be binned differently from the reference.
 *   - hysteresis / canny: if min_val <= 0 the reference's result depends on its scan order whenever a
 *     candidate is below min_val; that case returns CANNY_HIP_ERR_DOMAIN.  So does min_val > 255 >= max_val:
 *     the reference overwrites reached pixels with EDGE = 255 while its scan is still running, and a pixel the
 *     scan has not reached yet then fails `< minVal` and is zeroed again (src/utils.cpp:327-334) -- e.g.
 *     [[300,300,0,0]], min 300, max 100 gives [[255,0,0,0]].  find_edge_pixels rejects min_val > 255 likewise.
 *     (The reference's CLI only admits thresholds in [0,255], src/main.cpp:63-76.)
 *
 * Threading: a context is bound to one device and one stream and must be used by one host thread
 * at a time; different contexts may be used concurrently (one per GPU / per host thread).
 */
#ifndef CANNY_HIP_H
#define CANNY_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CANNY_HIP_VERSION 2900       /* 0.29.0: + image pyramids: pyrDown, pyrUp and whole pyramids of u8 planes */
/* 0.28.0: + grey-level morphology and median filtering of u8 planes */
/* 0.27.0: + morphological reconstruction of packed bit maps (seeded, fill holes, clear border) */
/* 0.26.0: + thinning of packed bit maps to one-pixel skeletons */
/* 0.25.0: + binarization: gray planes to packed bit maps (fixed, Otsu, adaptive) */
/* 0.24.0: + binary morphology on packed bit maps */
/* 0.23.0: + temporal fusion of aligned frames and change masks (0.22.0: + frame alignment) */
/* 0.21.0: + frame-to-frame motion from the corner matches (RANSAC) */
/* 0.20.0: + corner descriptors and Hamming matching between frames */
/* 0.19.0: + corners: Harris / Shi-Tomasi on the smoothed plane */
/* 0.18.0: + edge curves: the edge map linked into ordered chains */
/* 0.17.0: + contour shape measures: moments, convex hull, minimum-area rectangle */
/* 0.16.0: + chamfer template matching on the distance transform */
/* 0.15.0: + sub-pixel circle fits: least-squares refit of Hough circles from edgels */
/* 0.13.0: + sub-pixel edgels: position, gradient and strength per edge pixel */
/* 0.12.2: + canny_hip_selftest_launch_plan */
/* 0.12.1: + canny_hip_selftest_workspace */
/* 0.12.0: + polygon approximation of the contour chains, on the GPU */
/* 0.10.0: + outer contour chains of the finished map, traced on the GPU */
/* 0.11.0: + Hough circles: gradient rays, centre peaks, radius by support */
/* 0.9.1: + canny_hip_selftest_histogram, canny_hip_selftest_select */
/* 0.9.0: + Hough line segments: runs of edge pixels along each detected line */
/* 0.8.0: + exact Euclidean distance transform of the finished map: dist2, dist, nearest */
/* 0.7.0: + 8-connected components of the finished map: labels, stats, minimum-area filter */
/* 0.5.0: + edge point lists (CSR of pixel indices), compacted on the GPU */
/* 0.4.1: + canny_hip_selftest_sobel_pixel */
/* 0.4.0: + per-frame thresholds, explicit or chosen on the GPU (median / quantile) */
/* 0.3.0: + colour frame input (BGR / RGB / BGRA / RGBA -> gray on the GPU) */
/* 0.2.0: + batch u8 / bit maps, multi-GPU options, host_register, async dev_canny */
#define CANNY_HIP_MAX_WINDOW 129     /* largest Gaussian window (sigma <= 21.33) */

typedef struct canny_hip_ctx canny_hip_ctx;

enum canny_hip_status {
    CANNY_HIP_OK = 0,
    CANNY_HIP_ERR_INVALID = 1,     /* null pointer, non-positive size, bad sigma ... */
    CANNY_HIP_ERR_UNSUPPORTED = 2, /* size or window beyond what the kernels support */
    CANNY_HIP_ERR_NO_DEVICE = 3,   /* no usable HIP device: there is NO CPU fallback */
    CANNY_HIP_ERR_RUNTIME = 4,     /* HIP runtime failure, see canny_hip_last_error() */
    CANNY_HIP_ERR_DOMAIN = 5,      /* input outside the documented numeric domain */
    CANNY_HIP_ERR_NO_CONVERGE = 6  /* hysteresis propagation hit its iteration cap */
};

/* Stages for the per-stage HIP-event profile (canny_hip_profile_*). */
enum canny_hip_stage {
    CANNY_HIP_STAGE_GAUSSIAN = 0,
    CANNY_HIP_STAGE_SOBEL_NMS = 1,      /* the fused Sobel+NMS pass (roofline-graded kernel) */
    CANNY_HIP_STAGE_HYST_CLASSIFY = 2,
    CANNY_HIP_STAGE_HYST_PROPAGATE = 3,
    CANNY_HIP_STAGE_HYST_FINALIZE = 4,
    CANNY_HIP_STAGE_SOBEL = 5,
    CANNY_HIP_STAGE_NMS = 6,
    CANNY_HIP_STAGE_XY_GRADIENT = 7,
    CANNY_HIP_STAGE_TO_GRAY = 8,        /* the standalone colour -> gray pass (the fused one is timed as GAUSSIAN) */
    CANNY_HIP_STAGE_COUNT = 9,          /* the stages of the edge map itself, 0..8: unchanged, callers iterate over it */
    /* stages of what is derived from a finished map follow the map's own; canny_hip_profile_get and the bits of
     * "profile_stage_mask" take every value below CANNY_HIP_STAGE_END */
    CANNY_HIP_STAGE_COMPACT = 9,        /* edge point lists: the count, scan and scatter kernels */
    CANNY_HIP_STAGE_END = 10
};

/* Pixel layouts of the colour entry points (canny_hip_*_color, canny_hip_*to_gray): dense, interleaved, no row
 * padding -- channel k of pixel (r,c) of frame f at byte ((f*H + r)*W + c)*CH + k. */
enum canny_hip_layout {
    CANNY_HIP_GRAY8 = 0,  /* 1 byte: what every other entry point takes (identity) */
    CANNY_HIP_BGR8 = 1,   /* cv::Mat CV_8UC3 as VideoCapture / imread return it */
    CANNY_HIP_RGB8 = 2,   /* PPM, PIL, numpy */
    CANNY_HIP_BGRA8 = 3,  /* alpha ignored */
    CANNY_HIP_RGBA8 = 4
};

/* ---- library / context ------------------------------------------------------------------- */
int canny_hip_version(void);
const char *canny_hip_status_string(int status);
int canny_hip_device_count(int *count);

/* Creates a context on `device` with its own non-blocking stream. */
int canny_hip_ctx_create(canny_hip_ctx **ctx, int device);
void canny_hip_ctx_destroy(canny_hip_ctx *ctx);
/* Makes the context launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL
 * restores the context's own stream. */
int canny_hip_ctx_set_stream(canny_hip_ctx *ctx, void *hip_stream);
int canny_hip_ctx_device(const canny_hip_ctx *ctx);
/* Kernel-path selection, for A/B measurements and tests; every path gives identical results.
 *   "gaussian_path":  0 auto (default), 1 generic two-pass, 2 wave-marching (window <= 17 and width >= 4)
 *   "sobel_nms_path": 0 auto (default), 1 LDS-tiled, 2 wave-marching
 *   "gaussian_fma_div": 1 (default) / 0 -- single-fma division by the full-window weight (process-wide)
 *   "fuse_classify": 1 (default) / 0 -- canny(): the Sobel+NMS kernel writes the hysteresis bit-planes itself
 *                    (used when width % 8 == 0 and min_val >= 1; otherwise the separate kernels run)
 *   "smoothed_u8": 1 (default since round 3) / 0 -- canny(): the smoothed plane between the Gaussian and the fused Sobel+NMS
 *                    kernel is stored as bytes instead of shorts ((short)(sum/count) lies in [0,255],
 *                    src/utils.cpp:62): 5.25 instead of 7.25 algorithmic bytes per pixel through HBM.
 *                    Used when the fused path and the marching Gaussian apply, else ignored.
 *                    Same results bit for bit
 *   "hysteresis_tail": 1 (default) / 0 -- canny(): after two batch-wide propagation sweeps ONE launch with a workgroup
 *                    per frame runs the remaining sweeps to convergence (frames are independent, so a workgroup
 *                    barrier between a frame's sweeps is all the ordering needed).  The call then queues five
 *                    kernels and returns without waiting: no per-sweep launches, no host round trip.  Used for
 *                    frames of up to 4096 tiles of 64x64 (a 4K frame has 2040); 0 = the multi-launch scheme whose
 *                    host polls for convergence.  "tune_hyst_tail_after": 2 (default), 1..4 -- how many sweeps run
 *                    batch-wide before the tail kernel takes over
 *   "overlap_hysteresis": 0 (default) / 1 -- canny() on 16 or more frames: the propagation sweeps of the first half
 *                    of the batch run on a second stream beside the Sobel+NMS kernel of the second half
 *                    (measured 1.5 % slower on 128 x 4K, kept for A/B)
 *   "tune_batch_workers", "tune_batch_chunk_mb", "tune_batch_chunk_frames", "tune_batch_pipe_mode":
 *                    canny_hip_canny_batch's pipelines (host threads), the chunk size in megabytes of input or in
 *                    frames (frames win) and the stream structure of a pipeline (1 = upload, compute and download
 *                    stream chained by events, 2 = one in-order stream); 0 (default) = automatic: ONE three-stream
 *                    pipeline x 24 MB chunks, for pinned and for ordinary caller memory alike (round 3: pageable input
 *                    is staged by the library's thread pool, the output is written by it: "tune_batch_compact"; with
 *                    tune_batch_compact = 1 pageable buffers fall back to six single-stream pipelines x 8 MB).  HIP multiplexes a process's streams onto 4 hardware queues by
 *                    default (GPU_MAX_HW_QUEUES): a host application with many streams of its own should raise that
 *                    limit, or the three streams of the pipeline end up sharing a queue and serialise
 *   "stream_overlap": 0 (default) / 1 -- canny_hip_dev_canny_stream: the sweeps left in flight run on a second,
 *                    high-priority stream beside the next call's Gaussian instead of in order before it
 *                    (no gain on 128 x 4K batches, kept for A/B)
 *   "tune_sobel_seg": rows per wave segment of the marching Sobel+NMS kernel, 0 = automatic
 *   "tune_batch_compact": 0 (default) the s16 / u8 maps of the batch calls cross PCIe as 1-bit maps and are expanded
 *       into the caller's plane by host threads ("tune_batch_expand_threads": 0 = automatic, up to 8); 1 = the map
 *       itself is downloaded (rounds 1-2).  Same planes bit for bit
 *   "tune_sobel_px": 0 (default) 8 pixels per lane, 1 four pixels per lane (process-wide; the packed-i16 kernel only)
 *   "tune_sobel_variant": 0 (default) automatic -- the f32 marching arithmetic (4 waves per SIMD) for the fused
 *       Sobel+NMS+classify kernel of canny(), round 2's packed-i16 arithmetic (3 waves per SIMD) for the s16 -> s16
 *       stage kernel --, 1 packed-i16 everywhere, 2 f32 everywhere; same results bit for bit; process-wide
 *   "tune_plane_stores": 0 (default) the fused Sobel+NMS kernel parks a segment's plane bytes in LDS and writes
 *                    them as whole words after its last row, 1 direct byte stores (process-wide)
 *   "tune_gaussian_variant": 0 (default) symmetric-tap marching kernel, systolic row pass (the running sums travel
 *                    between lanes), row-pass products looked up in an LDS table; 1 LDS-ring marching kernel; 2
 *                    symmetric-tap kernel that multiplies and fetches its neighbours' products; 3 product-fetching row
 *                    pass with the table (the default of rounds 2-3); 4 systolic row pass that multiplies; same
 *                    results bit for bit (process-wide)
 *   "tune_gaussian_seg": approximate rows per wave segment of the marching Gaussian, 0 = automatic (process-wide)
 *   "tune_finalize_mode": 0 (default) row-major hysteresis finalize, 1 tile-patch finalize (process-wide)
 *   "profile_stage_mask": bit s set = stage s (CANNY_HIP_STAGE_*) gets an event pair while profiling is enabled;
 *                    0 (default) = all stages.  Every pair costs a few microseconds of stream time, so a timed
 *                    region that needs one kernel's duration enables that stage only.
 *   "profile_sample_interval": N >= 1 (default 1): only every N-th launch group of a stage gets its event pair
 *   "gray_rule": colour input -> gray, gray = (wb*B + wg*G + wr*R + 2^(s-1)) >> s with
 *                    0 (default) OpenCV cvtColor(*2GRAY) on CV_8U: (1868 B + 9617 G + 4899 R + 8192) >> 14,
 *                    1 PIL Image.convert('L'):                    (7471 B + 38470 G + 19595 R + 32768) >> 16
 *                    (the two differ on 39,135 of the 2^24 (R,G,B) triples)
 *   "fuse_gray": 1 (default) / 0 -- colour canny(): the marching Gaussian of the u8 smoothed path converts the colour rows
 *                    as it loads them (windows 3..9, width >= 4, default kernel variant); 0 = a standalone conversion
 *                    pass always runs first (A/B, tests).  Same results bit for bit */
int canny_hip_ctx_set_option(canny_hip_ctx *ctx, const char *name, int value);
/* Reads back "gray_rule", "fuse_gray", the read-only "last_canny_fused_gray" (1 if the context's last colour canny call
 * really ran the fused Gaussian), "smoothed_u8", "fuse_classify", "hysteresis_tail", "gaussian_path", "sobel_nms_path", "tune_batch_compact",
 * the read-only "batch_expand_threads" (threads of the expansion pool once a batch call has created it) and the read-only
 * "last_canny_smoothed_u8": 1 if the context's last canny call really ran on the u8 smoothed plane (the option is a
 * request: windows beyond 17, asymmetric taps and shapes the fused kernel does not take fall back to the s16 plane).
 * bench.py uses it to price the kernel it timed with the bytes that kernel moved. */
int canny_hip_ctx_get_option(const canny_hip_ctx *ctx, const char *name, int *value);
int canny_hip_synchronize(canny_hip_ctx *ctx);
/* Text of the last HIP runtime error seen by this context ("" if none). */
const char *canny_hip_last_error(const canny_hip_ctx *ctx);
/* Number of propagation sweeps that did work in the last hysteresis / canny call (diagnostic).  After a call that only
 * queued its kernels (see canny_hip_dev_canny) the count still lives on the device: the getter then copies it out and
 * SYNCHRONISES the context's stream, hence the non-const context. */
int canny_hip_last_hysteresis_iterations(canny_hip_ctx *ctx);

/* ---- device / pinned memory helpers (for hosts without their own HIP allocator) ----------- */
int canny_hip_malloc(canny_hip_ctx *ctx, void **dev_ptr, size_t bytes);
int canny_hip_free(canny_hip_ctx *ctx, void *dev_ptr);
int canny_hip_host_alloc(canny_hip_ctx *ctx, void **host_ptr, size_t bytes); /* pinned */
int canny_hip_host_free(canny_hip_ctx *ctx, void *host_ptr);
/* Page-locks / releases memory the caller allocated itself (the reference's frames are `new[]` arrays and cv::Mat
 * data, src/main.cpp:111-137): registered buffers are DMA'd in place by the batch entry points, exactly like
 * canny_hip_host_alloc memory.  Register once, not per call (~22 ms per GB). */
int canny_hip_host_register(canny_hip_ctx *ctx, void *host_ptr, size_t bytes);
int canny_hip_host_unregister(canny_hip_ctx *ctx, void *host_ptr);
int canny_hip_memcpy_h2d(canny_hip_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int canny_hip_memcpy_d2h(canny_hip_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);

/* ---- stage entry points on HOST buffers (synchronous; one frame) --------------------------- */
/* createGaussianKernel: host-only.  taps must hold `cap` floats; *window receives 1+2*ceil(3*sigma). */
int canny_hip_gaussian_kernel(float sigma, float *taps, int cap, int *window);
int canny_hip_gaussian(canny_hip_ctx *ctx, const unsigned char *img, float sigma, int height, int width,
                       short *result);
int canny_hip_xy_gradient(canny_hip_ctx *ctx, const short *img, int height, int width, short *grad_x,
                          short *grad_y);
int canny_hip_sobel(canny_hip_ctx *ctx, const short *img, int height, int width, short *magnitude,
                    short *angle);
int canny_hip_nms(canny_hip_ctx *ctx, const short *magnitude, const short *angle, int height, int width,
                  short *result);
/* In place, like the reference. */
int canny_hip_hysteresis(canny_hip_ctx *ctx, short *edge_candidates, int height, int width, int min_val,
                         int max_val);
/* In place on both arrays; visited is one byte per pixel (C++ bool). */
int canny_hip_find_edge_pixels(canny_hip_ctx *ctx, short *edge_candidates, unsigned char *visited, int start,
                               int min_val, int max_val, int height, int width);
/* Whole pipeline; unlike the reference's canny() the {0,255} edge map is returned in `edges`. */
int canny_hip_canny(canny_hip_ctx *ctx, const unsigned char *img, float sigma, int min_val, int max_val,
                    int height, int width, short *edges);
/* n_frames contiguous frames in, n_frames edge maps out, frame i of the output = canny() of frame i (the
 * reference calls canny() once per captured frame, src/main.cpp:120-137).  The batch is cut into chunks; the
 * upload of chunk j+1, the kernels of chunk j and the download of chunk j-1 run concurrently on three streams
 * chained by events (BASELINE config 3).  Input frames in pinned / registered host memory (canny_hip_host_alloc, ...)
 * are DMA'd in place, ordinary (pageable) input is staged through pinned chunk buffers by the library's thread pool.
 * The finished maps cross PCIe as 1-bit maps and the same pool writes the caller's plane from them ("tune_batch_compact",
 * default), so the OUTPUT buffer needs no pinning: 48-53 Gpixel/s on 4K frames, bound by the upload (src/cuda.cu:83-101
 * moves every plane both ways in full). */
int canny_hip_canny_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                          int max_val, int height, int width, short *edges);
/* Same, but the edge maps come back as 8-bit planes (NOEDGE = 0, EDGE = 255: the values of src/utils.h:5-6
 * fit a byte).  Not in the reference: its edge map is the s16 plane hysteresis() works in (src/utils.cpp:478);
 * over PCIe that plane is two thirds of all bytes moved, so batches that only need the final map should take
 * this one. */
int canny_hip_canny_batch_u8(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                             int max_val, int height, int width, unsigned char *edges);
/* Same, with the edge maps as BIT maps: 1 = EDGE, 0 = NOEDGE, rows packed MSB-first (pixel 0 of a row is bit 7 of the
 * row's first byte, as in PBM "P4" files and numpy.packbits) and padded to whole bytes, so frame i occupies
 * height * ((width + 7) / 8) bytes at bits + i * that.  The map only ever holds two values (src/utils.h:5-6), so
 * nothing is lost, and the download shrinks from 2 bytes per pixel to 1/8: the batch then runs at the rate frames can be
 * UPLOADED (one byte per pixel).  Not in the reference; the next step after SURVEY.md 8(f) item 2. */
int canny_hip_canny_batch_bits(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                               int max_val, int height, int width, unsigned char *bits);
/* Shards n_frames by contiguous ranges over n_devices GPUs (devices 0..n_devices-1), one host thread and one
 * context per GPU, each running the batch pipeline above on its shard; no collective (BASELINE config 5: the
 * reference has no multi-GPU path, frames are independent).  n_devices <= 0 = all.  The per-device contexts
 * (pipelines, streams, staging) are created on first use and kept until canny_hip_multi_gpu_release(); each
 * shard's threads are bound to the CPUs local to its GPU (sysfs local_cpulist) for the duration of the call.
 * One sharded call runs at a time per process.  Pinned caller buffers are DMA'd in place (allocate them on
 * the right NUMA node for best results); pageable ones are staged by each shard's thread pool. */
int canny_hip_canny_multi_gpu(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                              int height, int width, short *edges, int n_devices);
int canny_hip_canny_multi_gpu_u8(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                                 int height, int width, unsigned char *edges, int n_devices);
int canny_hip_canny_multi_gpu_bits(const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                                   int height, int width, unsigned char *bits, int n_devices);
/* Process-wide options of the sharder: "tune_batch_workers" / "tune_batch_chunk_mb" / "tune_batch_chunk_frames" /
 * "tune_batch_pipe_mode"
 * (applied to every shard's pipeline), "numa_affinity" 1 (default) / 0, "allow_device_reuse" 0 (default) / 1:
 * n_devices may exceed the device count, shard s then runs on device s % count (exercises the sharder with N > 1
 * on a one-GPU box; no use in production). */
int canny_hip_multi_gpu_set_option(const char *name, int value);
/* Destroys the cached per-device contexts. */
int canny_hip_multi_gpu_release(void);
/* CPUs local to `device` in sysfs list form ("0-31,128-159"); CANNY_HIP_ERR_UNSUPPORTED if the platform does not say. */
int canny_hip_device_local_cpus(int device, char *buf, int cap);
/* Frame range [begin, end) of shard `rank` of `world` (what canny_hip_canny_multi_gpu and bench.py use). */
int canny_hip_shard_range(int n_frames, int rank, int world, int *begin, int *end);

/* ---- colour frame input (the reference's caller converts with cvtColor(frame, gray, COLOR_BGR2GRAY) before canny(),
 * src/main.cpp:113-114) -------------------------------------------------------------------------------------------
 * `layout` is an enum canny_hip_layout value, anything else is CANNY_HIP_ERR_INVALID; the rule is the context's "gray_rule".
 * Every _color call returns the same status and the same map as the gray entry point it mirrors would return on the
 * converted plane; CANNY_HIP_GRAY8 is accepted everywhere and is the identity.
 * Not (yet) covered -- follow-ups: the multi-GPU sharder, canny_hip_dev_canny_stream, device-side _u8 / _bits
 * variants, and converting pageable colour input on the host pool while it is staged (1 byte per pixel up instead
 * of 3). */
/* One frame, host buffers, synchronous: `gray` receives height*width bytes. */
int canny_hip_to_gray(canny_hip_ctx *ctx, const unsigned char *src, int layout, int height, int width,
                      unsigned char *gray);
/* canny_hip_canny on a colour frame (frames of 1 MP and more go through the batch pipeline as a batch of one). */
int canny_hip_canny_color(canny_hip_ctx *ctx, const unsigned char *src, int layout, float sigma, int min_val,
                          int max_val, int height, int width, short *edges);
/* canny_hip_canny_batch / _u8 / _bits on colour frames: chunks, pinned staging and uploads are sized in input bytes
 * (a chunk of colour frames holds fewer frames).  Pinned / registered input is DMA'd in place. */
int canny_hip_canny_batch_color(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames, float sigma,
                                int min_val, int max_val, int height, int width, short *edges);
int canny_hip_canny_batch_color_u8(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames, float sigma,
                                   int min_val, int max_val, int height, int width, unsigned char *edges);
int canny_hip_canny_batch_color_bits(canny_hip_ctx *ctx, const unsigned char *srcs, int layout, int n_frames,
                                     float sigma, int min_val, int max_val, int height, int width, unsigned char *bits);
/* Device buffers, asynchronous: n_frames colour frames -> n_frames gray planes (the standalone pass; d_src may have
 * any byte alignment). */
int canny_hip_dev_to_gray(canny_hip_ctx *ctx, const unsigned char *d_src, int layout, int height, int width,
                          int n_frames, unsigned char *d_gray);
/* The fused kernel alone: canny_hip_dev_gaussian_u8 of the converted plane, converted as the rows are loaded.
 * CANNY_HIP_ERR_UNSUPPORTED where it does not apply (where canny_hip_dev_gaussian_u8 does not, windows beyond 9, A/B
 * variants). */
int canny_hip_dev_gaussian_u8_color(canny_hip_ctx *ctx, const unsigned char *d_src, int layout, float sigma, int height,
                                    int width, int n_frames, unsigned char *d_result);
/* canny_hip_dev_canny on colour frames.
 * COMPLETION CONTRACT: d_edges is complete IN STREAM ORDER on the context's stream when the call has returned (work
 * queued on that stream afterwards sees the final map) and HOST-VISIBLE after canny_hip_synchronize() -- whatever path
 * ran.  Whether the call itself blocks the host depends on the shape: frames of <= 4096 hysteresis tiles (64x64 px)
 * with width % 8 == 0, min_val >= 1 and the option hysteresis_tail = 1 (default) only QUEUE their five kernels and
 * return; every other shape polls the propagation's convergence flag and returns when it has converged.  The context's
 * stream is non-blocking with respect to the legacy default stream: a hipMemcpy on the default stream does NOT wait for
 * it -- copy with canny_hip_memcpy_d2h (same stream), or synchronize first.  (A colour call that converts first queues
 * one kernel more.)  d_src may be reused once the context's stream has passed the call. */
int canny_hip_dev_canny_color(canny_hip_ctx *ctx, const unsigned char *d_src, int layout, float sigma, int min_val,
                              int max_val, int height, int width, int n_frames, short *d_edges);

/* ---- per-frame hysteresis thresholds -------------------------------------------------------------------------------
 * Frame f of a call gets its own pair (min_val[f], max_val[f]), stored at [2f], [2f+1] of a pair array.  Domain:
 * 1 <= min_val <= max_val <= 255 (everything the reference's CLI accepts except min_val = 0).  In it frame f's edge map is
 * bit-identical to canny_hip_canny(frame f, sigma, min_val[f], max_val[f]); promoted pixels are always 255.
 * Automatic rules, on a per-frame 257-bin histogram h[0..256] with N = sum(h) and the inverted-CDF quantile
 *     Q(q) = min { b : h[0] + ... + h[b] >= max(1, ceil((double)q * (double)N)) },  0 < q <= 1:
 *   CANNY_HIP_AUTO_MEDIAN    histogram of the smoothed plane (the Gaussian's output, 0..255); m = Q(0.5),
 *                            min_val = floor((double)low * m), max_val = floor((double)high * m); 0 <= low <= high.
 *                            The "auto_canny" idiom is low = 1 - s, high = 1 + s.
 *   CANNY_HIP_AUTO_QUANTILE  histogram of min(magnitude, 256) of the pre-NMS gradient magnitude (canny_hip_sobel's plane,
 *                            borders included); min_val = Q(low), max_val = Q(high); 0 < low <= high <= 1 (skimage's
 *                            use_quantiles).
 * then min_val = clamp(min_val, 1, 255), max_val = clamp(max_val, min_val, 255) (a black frame gets (1, 1)).  low and high
 * are widened to double exactly and all arithmetic is IEEE double, on the host and on the device.  An unknown rule, low /
 * high outside these ranges, NaN or infinity: CANNY_HIP_ERR_INVALID.  Every other status is as for canny_hip_canny.
 * The histogram and select passes are timed as CANNY_HIP_STAGE_HYST_CLASSIFY.
 * Not (yet) covered -- follow-ups: colour input, u8 / bit-map output, the multi-GPU sharder. */
enum canny_hip_auto_rule { CANNY_HIP_AUTO_MEDIAN = 1, CANNY_HIP_AUTO_QUANTILE = 2 };
/* Host-only: the selection rule on one 257-bin histogram (tests; callers with histograms of their own).
 * CANNY_HIP_ERR_INVALID also for an empty histogram. */
int canny_hip_auto_thresholds_from_histogram(const unsigned int *hist257, int rule, float low, float high, int *min_val,
                                             int *max_val);
/* canny_hip_dev_canny with per-frame pairs from a DEVICE array of 2 * n_frames ints; entries outside the domain are
 * clamped as above.  Same completion contract as canny_hip_dev_canny. */
int canny_hip_dev_canny_thresholds(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, const int *d_thresholds,
                                   int height, int width, int n_frames, short *d_edges);
/* canny_hip_dev_canny with the pairs chosen per frame on the GPU by `rule`; nothing is read back to the host.
 * d_thresholds: device array of 2 * n_frames ints receiving the pairs used, or NULL. */
int canny_hip_dev_canny_auto(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int rule, float low, float high,
                             int height, int width, int n_frames, short *d_edges, int *d_thresholds);
/* canny_hip_canny_batch with per-frame pairs from a HOST array of 2 * n_frames ints.  Pairs outside the domain are
 * CANNY_HIP_ERR_INVALID, and then nothing is written. */
int canny_hip_canny_batch_thresholds(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma,
                                     const int *thresholds, int height, int width, short *edges);
/* canny_hip_canny_batch with automatic per-frame pairs.  thresholds: HOST array of 2 * n_frames ints receiving the pairs
 * used, or NULL. */
int canny_hip_canny_batch_auto(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int rule,
                               float low, float high, int height, int width, short *edges, int *thresholds);

/* ---- stage entry points on DEVICE buffers (asynchronous on the context's stream) ----------- */
/* All planes hold n_frames contiguous frames.  Workspace is owned and grown by the context. */
int canny_hip_dev_gaussian(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int height, int width,
                           int n_frames, short *d_result);
int canny_hip_dev_xy_gradient(canny_hip_ctx *ctx, const short *d_img, int height, int width, int n_frames,
                              short *d_grad_x, short *d_grad_y);
int canny_hip_dev_sobel(canny_hip_ctx *ctx, const short *d_img, int height, int width, int n_frames,
                        short *d_magnitude, short *d_angle);
int canny_hip_dev_nms(canny_hip_ctx *ctx, const short *d_magnitude, const short *d_angle, int height, int width,
                      int n_frames, short *d_result);
/* Fused Sobel + NMS: smoothed s16 in, suppressed magnitude s16 out; magnitude and angle never reach
 * HBM (4 algorithmic bytes per pixel).  d_smoothed must lie in [0,255] (gaussian output). */
int canny_hip_dev_sobel_nms(canny_hip_ctx *ctx, const short *d_smoothed, int height, int width, int n_frames,
                            short *d_nms);
/* The two kernels of canny()'s "smoothed_u8" path on their own (tests, A/B): the Gaussian storing bytes
 * and the fused Sobel+NMS reading them (3 algorithmic bytes per pixel).
 * CANNY_HIP_ERR_UNSUPPORTED where the marching kernels do not apply (window > 17, width < 4, asymmetric taps, A/B
 * variants). */
int canny_hip_dev_gaussian_u8(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int height, int width,
                              int n_frames, unsigned char *d_result);
int canny_hip_dev_sobel_nms_u8in(canny_hip_ctx *ctx, const unsigned char *d_smoothed, int height, int width,
                                 int n_frames, short *d_nms);
/* In place.  Blocks the host until propagation has converged (it polls a device flag). */
int canny_hip_dev_hysteresis(canny_hip_ctx *ctx, short *d_edge_candidates, int height, int width, int n_frames,
                             int min_val, int max_val);
/* gaussian -> fused sobel+nms -> hysteresis over n_frames resident frames.
 * COMPLETION CONTRACT: d_edges is complete IN STREAM ORDER on the context's stream when the call has returned (work
 * queued on that stream afterwards sees the final map) and HOST-VISIBLE after canny_hip_synchronize() -- whatever path
 * ran.  Whether the call itself blocks the host depends on the shape: frames of <= 4096 hysteresis tiles (64x64 px)
 * with width % 8 == 0, min_val >= 1 and the option hysteresis_tail = 1 (default) only QUEUE their five kernels and
 * return; every other shape polls the propagation's convergence flag and returns when it has converged.  The context's
 * stream is non-blocking with respect to the legacy default stream: a hipMemcpy on the default stream does NOT wait for
 * it -- copy with canny_hip_memcpy_d2h (same stream), or synchronize first. */
int canny_hip_dev_canny(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                        int height, int width, int n_frames, short *d_edges);
/* canny() for a STREAM of batches -- the reference's capture loop (src/main.cpp:120-137: canny() on one frame
 * after the other) with resident batches in place of frames.  Same results as canny_hip_dev_canny, but the call
 * ALWAYS returns with the batch's hysteresis sweeps still queued, also for the shapes whose plain call has to poll the
 * convergence flag (large frames, hysteresis_tail = 0): that host round trip (which idles the GPU for ~20 us) happens
 * in the next call, after that call has queued its Gaussian.  d_edges of call i
 * is complete -- for work queued on the context's stream and, after a synchronize, for the host -- once call i+1
 * or canny_hip_dev_canny_stream_flush() has returned; until then the caller must neither read nor free it.
 * d_img may be reused as soon as the context's stream has passed the call.  Every other compute entry point of
 * the context, ctx_set_stream, synchronize and destroy flush first, so mixing the two kinds of call is safe
 * (canny_hip_memcpy_* do not flush: copying batch i-1 out while batch i is in flight is the point).  Shapes the fused Sobel+NMS+classify kernel
 * does not take (width % 8 != 0, min_val < 1) run as a plain canny_hip_dev_canny. */
int canny_hip_dev_canny_stream(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges);
int canny_hip_dev_canny_stream_flush(canny_hip_ctx *ctx);
/* Same with an 8-bit edge map (0 / 255) as output; the s16 map is kept in a context workspace and narrowed
 * by one more elementwise kernel (this entry point exists for transfers, not for speed on the device). */
int canny_hip_dev_canny_u8(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                           int height, int width, int n_frames, unsigned char *d_edges);
/* ... and with a bit map as output (layout as canny_hip_canny_batch_bits: n_frames * height * ((width + 7) / 8) bytes). */
int canny_hip_dev_canny_bits(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                             int height, int width, int n_frames, unsigned char *d_bits);

/* ---- edge point lists ------------------------------------------------------------------------------------------------
 * The pixels of an edge map as INDICES -- what a Hough transform, RANSAC fitting or contour following start from
 * (np.flatnonzero(edges), cv::findNonZero(edges)); the reference's own convention: findEdgePixels(..., start, ...), pixel
 * (r,c) at r*width+c.  A typical frame has a few percent of its pixels set.
 * For frame f of a call with edge map E_f (the map canny_hip_canny returns for that frame, bit for bit):
 *   P_f = the indices r*width + c of all pixels with E_f[r][c] != 0, ASCENDING (raster order), as unsigned int.
 * The batch result is CSR-shaped: offsets[0 .. n_frames] with offsets[0] = 0 and offsets[f+1] - offsets[f] = |P_f| --
 * always the TRUE counts -- and the lists concatenated densely in frame order: points[offsets[f] + k] = P_f[k].
 * `capacity` is the number of unsigned ints `points` holds.  Entries whose global position is >= capacity are not written,
 * nothing is ever written at or past points + capacity, and every entry below it is written as above: overflow shows as
 * offsets[n_frames] > capacity, and the prefix that fits is exact.  points == NULL with capacity == 0 is the legal
 * "counts only" call (per-frame edge density); points == NULL with capacity > 0 is CANNY_HIP_ERR_INVALID.
 * The output is deterministic: same input, same bytes (no atomics on the ordering path).
 * The list follows the MAP, not the plane it is derived from: max_val > 255 makes the reference zero every reached pixel
 * (src/utils.cpp:336-340), so every list is then empty.  Statuses are those of canny_hip_dev_canny for the same arguments
 * (CANNY_HIP_ERR_DOMAIN for min_val <= 0, ...), and on a status other than OK neither points nor offsets are written.
 * The kernels are timed as CANNY_HIP_STAGE_COMPACT.
 * Not (yet) covered -- follow-ups: the overlapped three-stream batch pipeline (canny_hip_canny_points uploads the whole batch,
 * then computes), the multi-GPU sharder, colour input, per-frame / automatic thresholds, (x, y) pair output, and skipping
 * the s16 map's write when only the points are wanted. */
/* Device buffers, asynchronous; completion contract as canny_hip_dev_canny: d_points, d_offsets (and d_edges) are complete
 * in stream order on the context's stream when the call has returned.  d_edges receives the s16 map exactly as
 * canny_hip_dev_canny writes it, or is NULL (a context workspace then holds it).  d_offsets: n_frames + 1 entries. */
int canny_hip_dev_canny_points(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, unsigned int *d_points,
                               unsigned long long capacity, unsigned long long *d_offsets);
/* The compaction alone, on a device bit map in the layout of canny_hip_dev_canny_bits (rows MSB-first, padded to bytes;
 * d_bits may have any byte alignment): for callers who already hold bit maps.  The padding bits of a row are ignored,
 * whatever they hold.  Asynchronous. */
int canny_hip_dev_points_from_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                   unsigned int *d_points, unsigned long long capacity, unsigned long long *d_offsets);
/* Host buffers, synchronous: upload, canny, count; the offsets come down, then only min(offsets[n_frames], capacity) points
 * are compacted and downloaded -- a few percent of a plane crosses PCIe instead of the plane. */
int canny_hip_canny_points(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, unsigned int *points, unsigned long long capacity,
                           unsigned long long *offsets);
/* Host-only, needs no device: the same rule on ONE host bit map (what a caller of canny_hip_canny_batch_bits runs on the
 * maps it received); *count receives the true count. */
int canny_hip_points_from_bits(const unsigned char *bits, int height, int width, unsigned int *points,
                               unsigned long long capacity, unsigned long long *count);

/* ---- sub-pixel edgels ---------------------------------------------------------------------------------------------------
 * One record per edge pixel: its position along the gradient to 1/256 pixel, its gradient pair, its gradient magnitude to
 * 1/16 grey level and its direction -- what a least-squares line or circle fit, a calibration target or a stereo match
 * starts from.  The rule is all integers, so the records are the same bytes on every run and every machine;
 * tests/edgels_rule.py restates it in numpy / Python ints, DESIGN.md section 23 describes the kernels.
 * Input: one plane P per frame, unsigned char or short, height and width >= 2 (the smoothed plane of the detector: what
 * canny_hip_dev_gaussian writes, or any u8 / s16 plane), and one pixel (x, y).
 *   1. Gradient.  (gx, gy) is the reference's 3x3 pair at (x, y) with its border rules (gx clamps columns and drops rows
 *      outside the frame, gy clamps rows and drops columns) and its wrap through short: what canny_hip_xy_gradient returns.
 *      M(gx, gy) = (unsigned)(gx * gx) + (unsigned)(gy * gy) <= 2^31.  mag_q4 = floor(sqrt(256 * M)), EXACT: r * r <=
 *      256 * M < (r + 1) * (r + 1) in 64 bits, r < 2^20 -- the magnitude in 1/16 grey level.
 *   2. Direction: OpenCV's integer octant test (tan 22.5 deg = 13573 / 2^15), NOT the reference's float atan2 bins.
 *      ax = |gx|, ay = |gy|, t22 = ax * 13573, y15 = ay << 15, t67 = t22 + (ax << 16), unsigned, all below 2^32.
 *        gx = gy = 0       : dir 0, not refined
 *        y15 < t22         : dir 0, step (dx, dy) = (1, 0)
 *        y15 > t67         : dir 2, step (0, 1)
 *        otherwise         : gx and gy of the same sign: dir 1, step (1, 1); else dir 3, step (1, -1)
 *   3. Offset.  b = mag_q4 at (x, y), a = mag_q4 at (x - dx, y - dy), c = mag_q4 at (x + dx, y + dy), each neighbour's own
 *      pair from step 1 with its own border rules.  Dn = 2 * b - a - c.  The edgel is REFINED iff both neighbours lie inside
 *      the frame, the gradient is not zero, b >= a, b >= c and Dn > 0; then
 *        t_q8 = sgn(c - a) * ((256 * |c - a| + Dn) / (2 * Dn))      (floor division)
 *      -- the peak of the parabola through the three magnitudes, rounded half away from zero, in 1/256 of the step; b >=
 *      max(a, c) gives |t_q8| <= 128.  Not refined: t_q8 = 0.
 *   4. Record: CANNY_HIP_EDGEL_INTS = 4 32-bit words, 16 bytes, stored as a unit:
 *        word 0: x_q8 = 256 * x + t_q8 * dx  (int)
 *        word 1: y_q8 = 256 * y + t_q8 * dy  (int)
 *        word 2: (unsigned short)gx | (unsigned short)gy << 16
 *        word 3: mag_q4 in bits 0-23, dir in bits 24-25, CANNY_HIP_EDGEL_REFINED (bit 28), CANNY_HIP_EDGEL_INVALID (bit 31)
 *      An INVALID record answers an index >= height * width (possible in the index-list forms only): its other 127 bits are
 *      zero, and such an index never becomes an address.
 * The reference's non-maximum suppression decides by float atan2 bins, and for its bins 45 and 135 it compares the two
 * neighbours ALONG the edge (the up-right / down-left pair for a gradient that points down-right).  So a pixel of Canny's
 * own map need not be a maximum along this rule's step.  Those pixels come back unrefined, at the pixel centre, with their
 * gradient: that is deliberate -- the record says what the plane says, the map only chooses the pixels.
 * Records: 16-byte aligned buffers of `capacity` records.  Nothing is stored at or past capacity records.
 * The two parts are timed by canny_hip_edgels_profile_get (CANNY_HIP_EDGEL_PART_*); with "profile_stage_mask" they go by
 * bit 30 together with the polygon parts.
 * Not (yet) covered -- follow-ups: true-direction (Devernay) interpolation between neighbours in place of the quantised
 * step; colour, per-frame-threshold and automatic-threshold forms; the three-stream batch pipeline and the sharder;
 * least-squares refits of circles from edgels (lines and segment end points: the line fits below); dropping the s16
 * map's store when only edgels are wanted. */
#define CANNY_HIP_EDGEL_INTS 4
#define CANNY_HIP_EDGEL_MAG_MASK 0x00ffffffu
#define CANNY_HIP_EDGEL_DIR_SHIFT 24
#define CANNY_HIP_EDGEL_REFINED 0x10000000u
#define CANNY_HIP_EDGEL_INVALID 0x80000000u
enum canny_hip_edgel_part {
    CANNY_HIP_EDGEL_PART_LAYOUT = 0, /* count + scan of the map's rows */
    CANNY_HIP_EDGEL_PART_REFINE = 1, /* the records */
    CANNY_HIP_EDGEL_PARTS = 2
};
/* canny_hip_dev_canny unchanged (d_edges: the s16 map, or NULL), then count + scan as canny_hip_dev_canny_points, then one
 * record per edge pixel in that call's order (ascending r * width + c per frame, CSR over the batch), from the converged
 * strong plane and the smoothed plane the call left on the context.  d_offsets[0 .. n_frames] always holds the true counts;
 * d_edgels == NULL with capacity == 0 is the counts-only call.  d_points (optional, capacity unsigned ints) receives the
 * indices canny_hip_dev_canny_points would write.  max_val > 255 empties every list.  Asynchronous, same stream, no host
 * round trip, no atomics; statuses as canny_hip_dev_canny_points, CANNY_HIP_ERR_INVALID for a misaligned d_edgels. */
int canny_hip_dev_canny_edgels(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, int *d_edgels,
                               unsigned long long capacity, unsigned long long *d_offsets, unsigned int *d_points);
/* The rule at caller-chosen pixels: record q describes index d_points[q] of the frame whose range in d_point_offsets[0 ..
 * n_frames] (ascending, device) holds q -- a contour chain, a Hough segment's pixels, any list; entries are read as
 * unsigned.  Records at q >= capacity are not written.  d_plane: n_frames contiguous height x width planes, bytes if
 * plane_is_u8 else shorts; NULL = the smoothed plane the last canny_hip_dev_canny-family call on this context left (then
 * plane_is_u8 is ignored) -- CANNY_HIP_ERR_INVALID, with nothing queued, if no such call ran or its (n_frames, height,
 * width) differ.  Asynchronous; flushes a pending canny_hip_dev_canny_stream batch first. */
int canny_hip_dev_edgels_at(canny_hip_ctx *ctx, const void *d_plane, int plane_is_u8, int height, int width, int n_frames,
                            const unsigned int *d_points, const unsigned long long *d_point_offsets, int *d_edgels,
                            unsigned long long capacity);
/* Host buffers, synchronous: upload, canny, count; the offsets come down, then only min(offsets[n_frames], capacity)
 * records (and points, if asked for) are computed and downloaded. */
int canny_hip_canny_edgels(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int *edgels, unsigned long long capacity,
                           unsigned long long *offsets, unsigned int *points);
/* Host-only, needs no device: the rule in plain C++ on ONE host plane and one index list; edgels receives n_points
 * records. */
int canny_hip_edgels_from_plane(const void *plane, int plane_is_u8, int height, int width, const unsigned int *points,
                                unsigned long long n_points, int *edgels);
/* Test hook: the device arithmetic of the kernels on arrays.  (a) d_gx, d_gy (n_pairs shorts each) -> d_mag (mag_q4) and
 * d_dir; (b) d_abc (n_triples x 3 unsigned ints, each < 2^20) -> d_t (t_q8) and d_refined (1 iff b >= a, b >= c and Dn >
 * 0).  Either part may be empty (count 0, pointers ignored).  Asynchronous. */
int canny_hip_dev_edgels_arith(canny_hip_ctx *ctx, const short *d_gx, const short *d_gy, size_t n_pairs,
                               unsigned int *d_mag, int *d_dir, const unsigned int *d_abc, size_t n_triples, int *d_t,
                               int *d_refined);

/* ---- Hough lines -------------------------------------------------------------------------------------------------------
 * The standard Hough line transform of a finished edge map, per frame of a batch, on the GPU, in stream order, with no host
 * round trip: cv::HoughLines semantics (accumulator, local-maximum peaks, strongest lines first), i.e. OpenCV's
 * HoughLinesStandard restated without its build-dependent parts, so that a few lines of numpy (tests/hough_rule.py) reproduce
 * every accumulator cell and every returned line bit for bit.  THE RULE:
 * All float arithmetic is IEEE binary32, round to nearest even, not contracted (no fused multiply-add).
 * Arguments: rho > 0, theta > 0 (finite), threshold (int), lines_max >= 1, 0 <= min_theta < max_theta <= (float)pi.
 *   Geometry (double): numangle = floor(((double)max_theta - (double)min_theta) / (double)theta) + 1; if numangle > 1 and
 *     |pi - (numangle - 1) * (double)theta| < (double)theta / 2 then numangle -= 1;
 *     numrho = rint_half_even((2.0 * (width + height) + 1.0) / (double)rho).   (3840 x 2160, rho 1, theta pi/180: 180 x 12001)
 *   Tables (host): irho = 1.0f / rho; float ang = min_theta, advanced by ang = ang + theta in float;
 *     tab_cos[n] = (float)(cos((double)ang) * (double)irho), tab_sin[n] likewise.  canny_hip_hough_tables returns them; they
 *     are the only place a transcendental function is used, so the device result depends on no libm.
 *   Votes: for every set pixel (y, x) = (row, column) of the frame's map and every n < numangle
 *     r = (int)rint_half_even(fl(fl((float)x * tab_cos[n]) + fl((float)y * tab_sin[n]))) + (numrho - 1) / 2
 *     accum[(n + 1) * (numrho + 2) + r + 1] += 1.  accum is int, (numangle + 2) x (numrho + 2), its border row / column zero.
 *   Peaks: cell base = (n + 1) * (numrho + 2) + r + 1, 0 <= n < numangle, 0 <= r < numrho, is a peak iff
 *     a[base] > threshold && a[base] > a[base - 1] && a[base] >= a[base + 1] && a[base] > a[base - (numrho + 2)] &&
 *     a[base] >= a[base + (numrho + 2)].
 *   Order: peaks sorted by (votes descending, base ascending), a total order.  Frame f returns the first
 *     min(lines_max, n_peaks_f) of them; counts[f] = n_peaks_f, always the TRUE count.
 *   A line is returned three ways, in slot f * lines_max + k of each array: bases (unsigned), votes (int) and lines, two
 *     floats per slot: line_rho = ((float)r - (float)(numrho - 1) * 0.5f) * rho, line_theta = min_theta + (float)n * theta.
 *     Slots k >= min(lines_max, counts[f]) are not written.
 * The output is the same bytes on every run (integer atomics touch counters only; the final order comes from a sort on a
 * total order).  Any of lines, votes, bases, accum may be NULL; counts (n_frames ints) is mandatory.  d_accum, if given,
 * receives n_frames accumulators of (numangle + 2) * (numrho + 2) ints, border included; otherwise they live in a context
 * workspace of that size.
 * Statuses: rho / theta non-positive, NaN or infinite, a theta range outside [0, (float)pi] or empty, lines_max < 1, a NULL
 * counts -> CANNY_HIP_ERR_INVALID; lines_max > CANNY_HIP_HOUGH_MAX_LINES, an accumulator of 2^31 cells or more, numrho < 1
 * -> CANNY_HIP_ERR_UNSUPPORTED; nothing is written in either case.
 * "hough_path" (canny_hip_ctx_set_option): 0 automatic (default), 1 global integer atomics into a zeroed accumulator,
 *   2 accumulator rows in LDS.  The LDS form needs one row, numrho ints, to fit in the 160 KiB of a workgroup (numrho <=
 *   40960: every frame up to 8K at rho >= 0.6); beyond that 0 takes the global form and 2 is CANNY_HIP_ERR_UNSUPPORTED.  Same
 *   bytes either way.  "tune_hough_lds_kb": LDS budget of a vote workgroup in KiB (0 = automatic, 48), for A/B.
 * The three parts are timed by canny_hip_hough_profile_get (0 vote, 1 peaks, 2 select + sort).
 * Segment output (cv::HoughLinesP's use) is the next section, circles the one after it.
 * Not covered -- follow-ups: multi-scale srn / stn, weighted votes, the three-stream batch pipeline, the multi-GPU sharder,
 * colour and automatic-threshold variants. */
#define CANNY_HIP_HOUGH_MAX_LINES 4096 /* largest lines_max: the 64-bit sort keys of one frame fit in LDS */
/* Host-only, no device needed. */
int canny_hip_hough_geometry(int height, int width, float rho, float theta, float min_theta, float max_theta,
                             int *numangle, int *numrho);
int canny_hip_hough_tables(float rho, float theta, float min_theta, int numangle, float *tab_cos, float *tab_sin);
/* (line_rho, line_theta) of an accumulator cell, as the device writes them. */
int canny_hip_hough_line_of(unsigned int base, int numrho, float rho, float theta, float min_theta, float *line_rho,
                            float *line_theta);
/* From a CSR point list as canny_hip_dev_canny_points writes it: d_points must hold all d_offsets[n_frames] entries (a list
 * truncated by its capacity is not a valid input).  An index >= height * width is not a pixel: it casts no vote and causes
 * no access (what the result then means is up to the caller; the call stays memory-safe).  Asynchronous. */
int canny_hip_dev_hough_points(canny_hip_ctx *ctx, const unsigned int *d_points, const unsigned long long *d_offsets,
                               int n_frames, int height, int width, float rho, float theta, int threshold, int lines_max,
                               float min_theta, float max_theta, float *d_lines, int *d_votes, unsigned int *d_bases,
                               int *d_counts, int *d_accum);
/* From packed bit maps in the layout of canny_hip_dev_canny_bits (padding bits ignored).  Asynchronous. */
int canny_hip_dev_hough_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int height, int width,
                             float rho, float theta, int threshold, int lines_max, float min_theta, float max_theta,
                             float *d_lines, int *d_votes, unsigned int *d_bases, int *d_counts, int *d_accum);
/* canny_hip_dev_canny unchanged (d_edges as in canny_hip_dev_canny_points: the s16 map, or NULL), then the transform of its
 * map queued behind it on the same stream, read from the converged hysteresis bit-plane: no point list, no capacity.
 * Completion contract and statuses as canny_hip_dev_canny_points; the result follows the MAP (max_val > 255: all counts 0). */
int canny_hip_dev_canny_hough(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                              int height, int width, int n_frames, short *d_edges, float rho, float theta, int threshold,
                              int lines_max, float min_theta, float max_theta, float *d_lines, int *d_votes,
                              unsigned int *d_bases, int *d_counts, int *d_accum);
/* Host buffers, synchronous: upload, canny, transform; the counts come down, then only the filled slots of each frame. */
int canny_hip_canny_hough(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                          int max_val, int height, int width, float rho, float theta, int threshold, int lines_max,
                          float min_theta, float max_theta, float *lines, int *votes, unsigned int *bases, int *counts);

/* ---- Hough line segments ------------------------------------------------------------------------------------------------
 * Where on a detected line the edge is: the runs of edge pixels along each line of a list, per frame of a batch, on the GPU,
 * in stream order behind the Hough call, with no host round trip -- what cv::HoughLinesP is used for.  HoughLinesP itself
 * picks pixels with a random number generator and cannot be reproduced; this is a deterministic rule of the library's own,
 * which a few lines of numpy restate byte for byte (tests/hough_segments_rule.py).  THE RULE:
 * Inputs for one frame: its edge map E (height x width); rho, theta, min_theta, max_theta, hence numangle, numrho, tab_cos,
 *   tab_sin exactly as above; an ordered list of lines bases[0 .. K), accumulator cells; min_length >= 0, max_gap >= 0,
 *   exclusive in {0, 1}, segments_max >= 1.  All float arithmetic is binary32, round to nearest even, not contracted.
 *   1. Line: for each k, n = bases[k] / (numrho + 2) - 1, r = bases[k] % (numrho + 2) - 1.  A base with n outside
 *      [0, numangle) or r outside [0, numrho) is not a line: it yields no segment and causes no memory access.  Duplicate
 *      bases are allowed; each is a line of its own.
 *   2. Support: vote(x, y) = (int)rint_half_even(fl(fl((float)x * tab_cos[n]) + fl((float)y * tab_sin[n]))) + (numrho - 1) / 2
 *      -- the vote above, to the bit.  S_k = the pixels (y, x) set in the working map W with vote(x, y) == r: exactly the
 *      pixels that voted for the cell.  With exclusive = 0, W = E for every line, so |S_k| is the cell's vote count.
 *   3. Axes: the major axis is x if |tab_sin[n]| >= |tab_cos[n]| (compared as floats), else y.  t = the major coordinate,
 *      0 <= t < L (L = width or height), m = the minor one.  cnt[t] = the number of pixels of S_k at major position t,
 *      on[t] = cnt[t] > 0, lo[t] = the smallest m among them.
 *   4. Runs: take the on positions in ascending order; consecutive on positions t' < t'' belong to the same run iff
 *      t'' - t' - 1 <= max_gap (HoughLinesP's maxLineGap: up to max_gap consecutive off positions are bridged).  A run
 *      [ta, tb] is a segment iff tb - ta >= min_length (HoughLinesP's test on the larger coordinate difference);
 *      min_length = 0 keeps single pixels.
 *   5. Record: CANNY_HIP_SEGMENT_INTS = 6 ints x0, y0, x1, y1, k, support.  (x0, y0) is the pixel (ta, lo[ta]) mapped back
 *      to (x, y), (x1, y1) is (tb, lo[tb]) likewise, support = the sum of cnt[t] over ta <= t <= tb.  Both end points are set
 *      pixels of the map.
 *   6. Exclusive mode (exclusive = 1: a pixel serves one segment only, as in HoughLinesP): W starts as E; lines are handled
 *      in list order; after line k every pixel of S_k whose t lies inside a kept segment of line k is cleared from W, and
 *      line k + 1 sees the cleared map.  W is a private working copy: neither the context's hysteresis plane nor a caller's
 *      d_bits is ever written.
 *   7. Order and capacity: records sorted by (k ascending, ta ascending), a total order.  Frame f's records go to slots
 *      f * segments_max + j; only the first min(segments_max, total_f) are written; seg_counts[f] = total_f, always the TRUE
 *      count; later slots are not touched.  The result is the same bytes on every run.
 * In the device flavours the line list of frame f is d_bases[f * lines_max .. f * lines_max + min(lines_max,
 *   d_line_counts[f])): the arrays a Hough call leaves on the device.  Nothing comes back to the host between the two calls.
 * The kernels search the minor axis only near the line (a float estimate +- (0.7072 * rho + 2), widened by the float error
 *   of the largest product); inside that window the exact vote decides, and the tests show the result equal to the
 *   full-plane rule.  The rule itself knows no window.
 * Statuses: min_length < 0, max_gap < 0, exclusive not 0 / 1, segments_max < 1, lines_max < 1, a NULL mandatory pointer ->
 *   CANNY_HIP_ERR_INVALID; the Hough argument errors as above; n_frames * segments_max * 6 >= 2^31, lines_max >
 *   CANNY_HIP_HOUGH_MAX_LINES, a frame whose lines could hold 2^31 segments (lines * ceil(L / 2)), and exclusive mode with
 *   max(height, width) > 2^20 -> CANNY_HIP_ERR_UNSUPPORTED.  Nothing is written in either case.
 * Memory: exclusive mode keeps a private copy of the map in a context workspace (1 bit per pixel, tile padding included).
 * The parts are timed by canny_hip_hough_segments_profile_get (CANNY_HIP_SEGMENT_PART_*); with "profile_stage_mask" they
 *   are bits 19 .. 21.
 * Not covered -- follow-ups: randomised sampling as in HoughLinesP proper, decrementing the accumulator when pixels are
 * claimed, merging collinear segments of neighbouring cells, the three-stream batch pipeline, the multi-GPU sharder.
 * (Sub-pixel end points: the line fits, the section after next.) */
#define CANNY_HIP_SEGMENT_INTS 6
enum canny_hip_segment_part {
    CANNY_HIP_SEGMENT_PART_COUNT = 0,      /* exclusive = 0: every line walked, its segments counted; scan over the lines */
    CANNY_HIP_SEGMENT_PART_EMIT = 1,       /* exclusive = 0: every line walked again, the records stored */
    CANNY_HIP_SEGMENT_PART_EXCLUSIVE = 2,  /* exclusive = 1: the private copy, then one workgroup per frame, lines in order */
    CANNY_HIP_SEGMENT_PARTS = 3
};
/* Host-only, needs no device: the rule on ONE host bit map (layout of canny_hip_dev_canny_bits), a plain C++ walk of the
 * full plane.  bases may be NULL if n_lines == 0.  *count receives the true count. */
int canny_hip_hough_segments_from_bits(const unsigned char *bits, int height, int width, float rho, float theta,
                                       float min_theta, float max_theta, const unsigned int *bases, int n_lines,
                                       int min_length, int max_gap, int exclusive, int *segments, int segments_max,
                                       int *count);
/* Device bit maps (layout of canny_hip_dev_canny_bits, any byte alignment, padding bits ignored) and the line lists a Hough
 * call left on the device.  d_segments: n_frames * segments_max * 6 ints; d_seg_counts: n_frames ints.  Asynchronous. */
int canny_hip_dev_hough_segments_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int height, int width,
                                      float rho, float theta, float min_theta, float max_theta,
                                      const unsigned int *d_bases, const int *d_line_counts, int lines_max, int min_length,
                                      int max_gap, int exclusive, int *d_segments, int segments_max, int *d_seg_counts);
/* canny_hip_dev_canny_hough unchanged, then the segments queued behind it on the same stream, read from the converged
 * hysteresis bit-plane and from the bases that call wrote.  d_lines, d_votes, d_bases, d_line_counts, d_accum may be NULL
 * (bases and line counts then live in a context workspace); d_segments and d_seg_counts are mandatory.  The result follows
 * the MAP (max_val > 255: all counts 0).  Completion contract and statuses as canny_hip_dev_canny_hough. */
int canny_hip_dev_canny_hough_segments(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                       int max_val, int height, int width, int n_frames, short *d_edges, float rho,
                                       float theta, int threshold, int lines_max, float min_theta, float max_theta,
                                       float *d_lines, int *d_votes, unsigned int *d_bases, int *d_line_counts,
                                       int *d_accum, int min_length, int max_gap, int exclusive, int *d_segments,
                                       int segments_max, int *d_seg_counts);
/* Host buffers, synchronous: upload, canny, lines, segments; the counts come down first, then only the filled slots.
 * lines, votes, bases, line_counts may be NULL. */
int canny_hip_canny_hough_segments(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                   int max_val, int height, int width, float rho, float theta, int threshold,
                                   int lines_max, float min_theta, float max_theta, int min_length, int max_gap,
                                   int exclusive, float *lines, int *votes, unsigned int *bases, int *line_counts,
                                   int *segments, int segments_max, int *seg_counts);

/* ---- sub-pixel line fits --------------------------------------------------------------------------------------------------
 * For every segment record of the section above one LINE FIT record: the total-least-squares line through the sub-pixel
 * edgels of the segment's pixels, the sub-pixel end points on that line, and the residuals -- on the GPU behind the segments
 * call, on the same stream, with no host round trip and no atomics.  A Hough cell is only as fine as rho x theta; the fit
 * is typically 4 to 40 times closer to the edge (DESIGN.md section 24 has the table).  The rule is all integers, so the
 * records are the same bytes on every run and every machine; tests/line_fits_rule.py restates it in Python ints,
 * csrc/canny_line_fits_host.cpp in plain C++.  THE RULE:
 * Inputs for one frame: the edge map E; a plane P, unsigned char or short (the smoothed plane of the detector call, or a
 *   caller's plane), height and width >= 2; the Hough geometry and tables exactly as in the two sections above; the line
 *   list bases[0 .. K); the segment records of the section above, taken in their slots; options: bit 0 =
 *   CANNY_HIP_LINE_FIT_GATE, bit 1 = CANNY_HIP_LINE_FIT_REFINED_ONLY, any other bit -> CANNY_HIP_ERR_INVALID.
 * For segment j with record (x0, y0, x1, y1, k, support):
 *   1. Line.  (n, r) from bases[k] as in step 1 of the segments, the major axis as in their step 3; ta, tb = the major
 *      coordinates of (x0, y0) and (x1, y1).  The record is INVALID -- word 9 = CANNY_HIP_LINE_FIT_INVALID, the other
 *      eleven words zero -- if k lies outside [0, K), the base is not an accumulator cell, an end point lies outside the
 *      frame, or ta > tb.  That can happen only in the forms that take caller-made records; an invalid record causes no
 *      memory access beyond the record and the base.
 *   2. Pixels.  The set pixels of E with vote(x, y) == r (step 2 of the segments, to the bit) and major coordinate in
 *      [ta, tb].  E itself, NOT the working map W of exclusive mode: the fit takes what lies on the line inside the
 *      segment's extent, even where an earlier line claimed it.  So with exclusive = 1, n may exceed the record's support;
 *      with exclusive = 0 and options = 0, n == support.
 *   3. Edgels.  Each pixel yields its record of the edgel section from P, unchanged: (x_q8, y_q8), (gx, gy), refined.
 *      With GATE a pixel is used only if (gx, gy) != (0, 0) and
 *        4 * (gx * ddx + gy * ddy)^2 <= (gx^2 + gy^2) * (ddx^2 + ddy^2),  (ddx, ddy) = (x1 - x0, y1 - y0)
 *      -- gradients within 30 degrees of the segment's normal; |gx * ddx + gy * ddy| < 2^30, so the left side is below
 *      2^62 and the right below 2^31 * 2^29.  With REFINED_ONLY a pixel is used only if refined.  n = the used pixels.
 *   4. Moments, relative to the first end point: u = x_q8 - 256 * x0, v = y_q8 - 256 * y0.  Su, Sv, Suu, Suv, Svv exactly.
 *      A = n * Suu - Su^2, B = n * Suv - Su * Sv, C = n * Svv - Sv^2, exact (128 bits).  A, C >= 0.
 *      s = max(0, bitlength(max(A, C, |B|)) - 28); A, B, C >>= s, an arithmetic shift (floor).
 *   5. Direction.  D = A - C, E = 2 * B, h = isqrt(D^2 + E^2), the exact floor; |D| < 2^28, |E| <= 2^29, the argument
 *      below 2^59.  The fit is DEGENERATE if n < 2 or h == 0.  Otherwise w = (h + D, E) if D >= 0, else
 *      w = (|E|, (h - D) * sgn(E)) with sgn(0) = +1 -- the eigenvector of the larger eigenvalue in the form that does not
 *      cancel.  w is negated iff wx * ddx + wy * ddy < 0: the direction follows the record's order.
 *      Then w <<= k with k = 31 - bitlength(max(|wx|, |wy|)): the larger component gets exactly 31 bits (max(|wx|, |wy|)
 *      <= 2^28 * (1 + sqrt 5) < 2^30, so k >= 1, and it is not 0 because h > 0).  Without this step a short segment with
 *      small moments (len = 6, say) would get a "unit" direction that is off by a tenth.
 *      len = isqrt(wx^2 + wy^2) (2^30 <= len, argument below 2^63), dx_q30 = rdiv(wx * 2^30, len), dy_q30 likewise;
 *      rdiv(a, b) rounds to nearest, halves away from zero: sgn(a) * ((2 * |a| + b) / (2 * b)), floor division.  So
 *      dx_q30^2 + dy_q30^2 lies within 2^-28 of 2^60: the floor in len costs at most 2 / len <= 2^-29, the two roundings
 *      less than 2^-29 more.
 *   6. Centroid in 1/65536 px: mu = rdiv(256 * Su, n), mv = rdiv(256 * Sv, n); cx_q16 = 65536 * x0 + mu, cy_q16 likewise.
 *   7. Residuals and extent, a second pass over the same used pixels; all shifts arithmetic.  U = 256 * u - mu,
 *      V = 256 * v - mv; d_q8 = (V * dx_q30 - U * dy_q30 + 2^37) >> 38; p_q16 = (U * dx_q30 + V * dy_q30 + 2^29) >> 30.
 *      Sdd = the sum of d_q8^2 (unsigned 64 bits), maxd = max |d_q8|, pmin and pmax over p_q16.
 *      End point 0 = (cx_q16 + ((pmin * dx_q30 + 2^29) >> 30), cy_q16 + ((pmin * dy_q30 + 2^29) >> 30)); end point 1 the
 *      same with pmax.  pmin <= 0 <= pmax up to the rounding of the centroid.
 *   8. Record: CANNY_HIP_LINE_FIT_INTS = 12 32-bit words, 48 bytes:
 *        words 0-3: x0_q16, y0_q16, x1_q16, y1_q16 (the fitted end points, 1/65536 px)
 *        words 4-5: cx_q16, cy_q16                  words 6-7: dx_q30, dy_q30 (unit direction, 2^-30)
 *        word 8: n       word 9: maxd in bits 0-23, CANNY_HIP_LINE_FIT_DEGENERATE (bit 28), CANNY_HIP_LINE_FIT_INVALID (bit 31)
 *        words 10-11: Sdd, low word first.  The caller's RMS distance is sqrt(Sdd / n) / 256 px.
 *      A DEGENERATE record carries words 0-3 = 65536 * the record's own end points, words 4-5 = the centroid if n >= 1,
 *      else the first end point, words 6, 7, 10, 11 = 0, word 8 = n, maxd = 0.
 *   9. Order and capacity: the fit of segment slot f * segments_max + j goes to fit slot f * segments_max + j, for j <
 *      min(segments_max, seg_counts[f]); later slots are not touched.
 * Limits: max(height, width) <= CANNY_HIP_LINE_FIT_MAX_AXIS = 16384 and rho <= CANNY_HIP_LINE_FIT_MAX_RHO = 8, else
 *   CANNY_HIP_ERR_UNSUPPORTED with nothing written.  They keep every sum inside 64 bits:
 *     |u|, |v| <= 256 * 16383 + 128 < 2^22.01      (a pixel of the frame against an end point of the frame, |t_q8| <= 128)
 *     n <= 16384 * (sqrt(2) * 8 + 1) < 2^18        (the votes of one t with vote == r span less than sqrt(2) * rho + 1
 *                                                   minor coordinates: the vote moves by at least 1 / (rho * sqrt 2) per pixel)
 *     Suu, Svv, |Suv| <= n * u^2 < 2^18 * 2^44.02 < 2^63;   |Su|, |Sv| < 2^40.01;   A, C, |B| < 2^18 * 2^62.02 < 2^81
 *     |U|, |V| < 2^30.02 (a point against the centroid of points of the same frame), so |V * dx - U * dy| and
 *     |U * dx + V * dy| are at most 2^30 * sqrt(U^2 + V^2) < 2^60.6 (Cauchy-Schwarz; the direction has length 2^30);
 *     |d_q8| <= 256 * the frame's diagonal + 1 < 2^22.51, which fits the 24 bits of maxd, and with n <= 201716 < 2^17.63
 *     Sdd < 2^17.63 * 2^45.02 < 2^63.
 *   Frames under 2 x 2: CANNY_HIP_ERR_INVALID, as for the edgels.
 * The part is timed by canny_hip_line_fits_profile_get (CANNY_HIP_LINE_FIT_PART_FIT); with "profile_stage_mask" it goes by
 * bit 30 together with the polygon and edgel parts.
 * Not (yet) covered -- follow-ups: magnitude-weighted fits, merging collinear
 * segments, colour / automatic-threshold / batch-pipeline / sharder forms, keeping the used (u, v) pairs in LDS for the
 * second pass. */
#define CANNY_HIP_LINE_FIT_INTS 12
#define CANNY_HIP_LINE_FIT_GATE 1
#define CANNY_HIP_LINE_FIT_REFINED_ONLY 2
#define CANNY_HIP_LINE_FIT_MAXD_MASK 0x00ffffffu
#define CANNY_HIP_LINE_FIT_DEGENERATE 0x10000000u
#define CANNY_HIP_LINE_FIT_INVALID 0x80000000u
#define CANNY_HIP_LINE_FIT_MAX_AXIS 16384
#define CANNY_HIP_LINE_FIT_MAX_RHO 8.0f
enum canny_hip_line_fit_part {
    CANNY_HIP_LINE_FIT_PART_FIT = 0, /* the one kernel: both walks and the finishing arithmetic */
    CANNY_HIP_LINE_FIT_PARTS = 1
};
/* Host-only, needs no device: the rule in plain C++ on ONE host frame.  bits: the edge map in the layout of
 * canny_hip_dev_canny_bits; plane: height x width bytes if plane_is_u8 else shorts; numangle, numrho, tab_cos, tab_sin: what
 * canny_hip_hough_geometry and canny_hip_hough_tables return for the Hough arguments; bases[0 .. n_lines); segments:
 * n_segments records of 6 ints; fits receives n_segments records of 12 ints.  The support is found on the full plane. */
int canny_hip_line_fits_from_plane(const unsigned char *bits, const void *plane, int plane_is_u8, int height, int width,
                                   float rho, int numangle, int numrho, const float *tab_cos, const float *tab_sin,
                                   const unsigned int *bases, int n_lines, const int *segments, int n_segments,
                                   int options, int *fits);
/* Device bit maps (layout of canny_hip_dev_canny_bits, any byte alignment; the padding bits of a row are ignored, whatever
 * they hold), a device plane (bytes if plane_is_u8 else shorts, n_frames contiguous
 * planes) and the bases, line counts, segments and segment counts that the earlier calls left on the device.  d_plane ==
 * NULL means the smoothed plane the last canny_hip_dev_canny-family call on this context left, under the rule of
 * canny_hip_dev_edgels_at: CANNY_HIP_ERR_INVALID, nothing queued, if no such call ran or its shape differs.  d_fits:
 * n_frames * segments_max * 12 ints, 16-byte aligned.  Asynchronous. */
int canny_hip_dev_line_fits_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, const void *d_plane, int plane_is_u8,
                                 int n_frames, int height, int width, float rho, float theta, float min_theta,
                                 float max_theta, const unsigned int *d_bases, const int *d_line_counts, int lines_max,
                                 const int *d_segments, const int *d_seg_counts, int segments_max, int options,
                                 int *d_fits);
/* canny_hip_dev_canny_hough_segments unchanged, then the fits queued behind it on the same stream, read from the converged
 * strong bit-plane and the smoothed plane that call left on the context.  d_fits is mandatory; everything else as there.
 * max_val > 255: all segment counts are 0 and no fit is written. */
int canny_hip_dev_canny_hough_line_fits(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                        int max_val, int height, int width, int n_frames, short *d_edges, float rho,
                                        float theta, int threshold, int lines_max, float min_theta, float max_theta,
                                        float *d_lines, int *d_votes, unsigned int *d_bases, int *d_line_counts,
                                        int *d_accum, int min_length, int max_gap, int exclusive, int *d_segments,
                                        int segments_max, int *d_seg_counts, int options, int *d_fits);
/* Host buffers, synchronous, in the pattern of canny_hip_canny_hough_segments: the counts come down first, then only the
 * filled slots.  lines, votes, bases, line_counts, segments may be NULL; fits and seg_counts are mandatory. */
int canny_hip_canny_hough_line_fits(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                    int max_val, int height, int width, float rho, float theta, int threshold,
                                    int lines_max, float min_theta, float max_theta, int min_length, int max_gap,
                                    int exclusive, int options, float *lines, int *votes, unsigned int *bases,
                                    int *line_counts, int *segments, int segments_max, int *seg_counts, int *fits);
/* Test hook: the device finishing function (steps 4 to 6) on n_sets moment sets of 8 long longs (n, Su, Sv, Suu, Suv, Svv,
 * ddx, ddy), n <= 2^18 and the sums within the limits above; d_out receives 6 ints per set: words 4 to 8 of the record
 * for (x0, y0) = (0, 0), i.e. mu, mv, dx_q30, dy_q30, n, then CANNY_HIP_LINE_FIT_DEGENERATE or 0.  Asynchronous. */
int canny_hip_dev_line_fits_arith(canny_hip_ctx *ctx, const long long *d_moments, size_t n_sets, int *d_out);
/* Host-only, the same hook on the plain C++ restatement (host arrays). */
int canny_hip_line_fits_finish(const long long *moments, size_t n_sets, int *out);

/* ---- Hough circles -------------------------------------------------------------------------------------------------------
 * Circle detection on a finished edge map, per frame of a batch, on the GPU, in stream order, with no host round trip:
 * cv::HoughCircles(HOUGH_GRADIENT) semantics, i.e. OpenCV's HoughCirclesGradient with its build-dependent and sequential-float
 * parts replaced by integer arithmetic, so that a few lines of numpy (tests/hough_circles_rule.py) reproduce every accumulator
 * cell and every returned record byte for byte.  THE RULE:
 * All float arithmetic is IEEE binary32, round to nearest even, not contracted.
 * Arguments: 1 <= min_radius <= max_radius <= CANNY_HIP_CIRCLES_MAX_RADIUS; cell_shift in 0..3 (an accumulator cell is
 *     c = 1 << cell_shift pixels wide: OpenCV's dp = c); threshold (int, centre votes); support_threshold (int, pixels on the
 *     circle); min_dist (int >= 0 pixels, 0 disables it); centres_max in 1..CANNY_HIP_HOUGH_MAX_LINES.
 *   Gradient: (gx, gy) at a pixel is the 3x3 Sobel pair of the reference (calculateXYGradient, src/utils.cpp:106-187: gx clamps
 *     columns and drops rows outside the frame, gy clamps rows and drops columns).  The canny forms take it on the smoothed plane
 *     of that call; the bit-map forms read it from two caller-supplied s16 planes.
 *   Step: m = sqrt((float)(unsigned)(gx * gx + gy * gy)) -- the sum in unsigned 32-bit (it cannot overflow for s16 inputs), the
 *     conversion and the root each rounded once; sx = (int)rint_half_even((float)(gx * 1024) / m) (gx * 1024 is exact in
 *     binary32 for every s16 gx), sy likewise.  A pixel with gx = gy = 0 casts no vote.  canny_hip_hough_circles_step_of
 *     returns the pair.
 *   Votes: aw = ceil(width / c), ah = ceil(height / c); accum is int, (ah + 2) x (aw + 2), its border row / column zero (the
 *     shape convention of the line accumulator with ah for numangle, aw for numrho).  For every set pixel (y, x) = (row, column)
 *     with a non-zero gradient, every sign s in {+1, -1} and every k in min_radius .. max_radius:
 *       X = x * 1024 + s * k * sx, Y = y * 1024 + s * k * sy; px = X >> 10, py = Y >> 10 (arithmetic shift: floor);
 *       if 0 <= px < width and 0 <= py < height: accum[((py >> cell_shift) + 1) * (aw + 2) + (px >> cell_shift) + 1] += 1.
 *   Centres: the five-way peak rule and the order of the Hough lines apply unchanged: cell base = (ay + 1) * (aw + 2) + ax + 1 is
 *     a peak iff a[base] > threshold && a[base] > a[base - 1] && a[base] >= a[base + 1] && a[base] > a[base - (aw + 2)] &&
 *     a[base] >= a[base + (aw + 2)]; peaks sorted by (votes descending, base ascending); the first K = min(centres_max,
 *     n_peaks) are the candidates.  A candidate's centre in DOUBLED pixel coordinates is x2 = (2 * ax + 1) * c,
 *     y2 = (2 * ay + 1) * c: OpenCV's (ax + 0.5) * dp, kept as an integer.
 *   Radius: every set pixel (y, x) of the map (zero-gradient ones included, as in OpenCV) has d = (2x - x2)^2 + (2y - y2)^2 and
 *     falls into radius bin r, the integer with (2r - 1)^2 <= d < (2r + 1)^2.  Among the bins min_radius .. max_radius the
 *     candidate's radius is the one with the largest count[r] / r, compared in integers (count[q] * r > count[r] * q), the
 *     smaller r on a tie; support = count[radius].  A candidate is VALID iff support > support_threshold.
 *   Acceptance: the candidates in order; a valid one is accepted iff no earlier ACCEPTED one has
 *     (dx2)^2 + (dy2)^2 < (2 * min_dist)^2.
 *   Output: frame f writes its accepted circles to slots f * centres_max + j of circles, compactly and in candidate order,
 *     CANNY_HIP_CIRCLE_INTS = 6 ints each: x2, y2, radius, votes, support, base.  counts[f] = the number accepted -- always the
 *     true count, it cannot exceed centres_max; centre_counts[f] = the true n_peaks.  Later slots are not written.
 * The output is the same bytes on every run (integer adds commute; the order comes from a sort on a total order; the acceptance
 * pass is a defined sequence).  circles, centre_counts and accum may be NULL; counts (n_frames ints) is mandatory.  d_accum, if
 * given, receives n_frames accumulators of (ah + 2) * (aw + 2) ints, border included; otherwise they live in a context
 * workspace of that size, freed with the context.
 * Statuses: a bad radius range (min_radius < 1 or > max_radius), cell_shift outside 0..3, centres_max < 1, min_dist < 0, a NULL
 * counts, NULL gradient planes in the bit-map forms, height < 2 or width < 2 -> CANNY_HIP_ERR_INVALID; max_radius >
 * CANNY_HIP_CIRCLES_MAX_RADIUS, centres_max > CANNY_HIP_HOUGH_MAX_LINES, an accumulator of 2^31 cells or more (and a bound
 * on a cell's votes, DESIGN.md section 18, above 2^26: only max_radius > 797 with cell_shift 3 on a frame larger than
 * 1606 x 1606) -> CANNY_HIP_ERR_UNSUPPORTED; nothing is written in either case.  max_val > 255 follows the MAP: all counts 0.
 * The four parts are timed by canny_hip_hough_circles_profile_get (CANNY_HIP_CIRCLE_PART_*); with "profile_stage_mask" they
 *   are bits 26 .. 29.
 * Not covered -- follow-ups: an accumulator-tile vote in LDS, HOUGH_GRADIENT_ALT, sub-cell centre refinement, several radii per
 * centre, the three-stream batch pipeline, the multi-GPU sharder, colour and per-frame / automatic-threshold variants. */
#define CANNY_HIP_CIRCLES_MAX_RADIUS 1024
#define CANNY_HIP_CIRCLE_INTS 6
enum canny_hip_circle_part {
    CANNY_HIP_CIRCLE_PART_VOTE = 0,     /* accumulators zeroed; set pixels queued in LDS, Sobel pair, step, ray votes */
    CANNY_HIP_CIRCLE_PART_CENTRES = 1,  /* peaks, cut-off, ties, collect, sort: the candidates in order */
    CANNY_HIP_CIRCLE_PART_RADIUS = 2,   /* per candidate: radius histogram of its window of the map, best radius, support */
    CANNY_HIP_CIRCLE_PART_ACCEPT = 3,   /* per frame: validity, minimum distance, records and counts */
    CANNY_HIP_CIRCLE_PARTS = 4
};
/* Host-only, no device needed: the step of one gradient (s16 range), as the device computes it. */
int canny_hip_hough_circles_step_of(int gx, int gy, int *sx, int *sy);
/* Host-only, needs no device: the same rule on ONE host bit map (layout of canny_hip_canny_batch_bits) and its two gradient
 * planes (height * width shorts each), in plain C++.  circles (centres_max * 6 ints; only the accepted records are written),
 * centre_count and accum ((ah + 2) * (aw + 2) ints) may be NULL. */
int canny_hip_hough_circles_from_bits(const unsigned char *bits, const short *gx, const short *gy, int height, int width,
                                      int min_radius, int max_radius, int cell_shift, int threshold, int support_threshold,
                                      int min_dist, int centres_max, int *circles, int *count, int *centre_count,
                                      int *accum);
/* From packed bit maps in the layout of canny_hip_dev_canny_bits (padding bits ignored) and full gradient planes d_gx, d_gy
 * (n_frames * height * width shorts each).  Asynchronous. */
int canny_hip_dev_hough_circles_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, const short *d_gx, const short *d_gy,
                                     int n_frames, int height, int width, int min_radius, int max_radius, int cell_shift,
                                     int threshold, int support_threshold, int min_dist, int centres_max, int *d_circles,
                                     int *d_counts, int *d_centre_counts, int *d_accum);
/* canny_hip_dev_canny unchanged (d_edges as in canny_hip_dev_canny_points: the s16 map, or NULL), then the transform queued
 * behind it on the same stream: the map is read from the converged hysteresis bit-plane, the gradient is recomputed at the
 * edge pixels from the smoothed plane that call left on the device (bytes or shorts, whichever it ran with).  Completion
 * contract and statuses as canny_hip_dev_canny_points; the result follows the MAP (max_val > 255: all counts 0). */
int canny_hip_dev_canny_hough_circles(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                      int height, int width, int n_frames, short *d_edges, int min_radius, int max_radius,
                                      int cell_shift, int threshold, int support_threshold, int min_dist, int centres_max,
                                      int *d_circles, int *d_counts, int *d_centre_counts, int *d_accum);
/* Host buffers, synchronous: upload, canny, transform; the counts come down, then only the filled slots of each frame. */
int canny_hip_canny_hough_circles(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                  int max_val, int height, int width, int min_radius, int max_radius, int cell_shift,
                                  int threshold, int support_threshold, int min_dist, int centres_max, int *circles,
                                  int *counts, int *centre_counts);
/* The device's step arithmetic alone on n gradient pairs (device arrays; d_sx, d_sy receive n ints each): the hook of the
 * exhaustive test, which runs every pair of the Sobel domain through it.  Asynchronous. */
int canny_hip_dev_hough_circles_steps(canny_hip_ctx *ctx, const short *d_gx, const short *d_gy, size_t n, int *d_sx,
                                      int *d_sy);

/* ---- sub-pixel circle fits ------------------------------------------------------------------------------------------------
 * For every circle record of the section above one CIRCLE FIT record: the least-squares (Kasa) circle through the sub-pixel
 * edgels of the edge pixels in a band around the Hough circle, the mean-distance radius, the residuals and a mask of the
 * angular sectors that hold points -- on the GPU behind the circles call, on the same stream, with no host round trip and no
 * atomics.  A Hough circle is only as fine as its cell and its whole-pixel radius; the fitted centre is typically 5 to 100
 * times closer to the truth (DESIGN.md section 25 has the table).  The rule is all integers, so the records are the same
 * bytes on every run and every machine; tests/circle_fits_rule.py restates it in Python ints,
 * csrc/canny_circle_fits_host.cpp in plain C++.  THE RULE:
 * Inputs for one frame: the edge map E; a plane P, unsigned char or short (the smoothed plane of the detector call, or a
 *   caller's plane), height and width >= 2; the circle records (x2, y2, radius, votes, support, base) of the section above,
 *   taken in their slots; band in 0 .. CANNY_HIP_CIRCLE_FIT_MAX_BAND; trim_q8 >= 0 (0 = off); options: bit 0 =
 *   CANNY_HIP_CIRCLE_FIT_GATE, bit 1 = CANNY_HIP_CIRCLE_FIT_REFINED_ONLY, any other bit -> CANNY_HIP_ERR_INVALID.
 * For record j:
 *   1. Validity.  The record is INVALID -- word 4 = CANNY_HIP_CIRCLE_FIT_INVALID, the other seven words zero -- iff radius
 *      lies outside [1, CANNY_HIP_CIRCLES_MAX_RADIUS], x2 outside [0, 2 * width) or y2 outside [0, 2 * height).  This is
 *      decided before any access beyond the record; only caller-made records can be invalid.
 *   2. Pixels.  The set pixels of E with (2 * lo - 1)^2 <= d < (2 * (radius + band) + 1)^2, d = (2x - x2)^2 + (2y - y2)^2,
 *      lo = max(radius - band, 1): the bin rule of the circles, widened by band bins on each side.  With band = 0,
 *      options = 0 and trim_q8 = 0, n == support for every record the circle call produced.
 *   3. Edgels.  Each pixel yields its record of the edgel section from P, unchanged: (x_q8, y_q8), (gx, gy), refined.
 *      With GATE a pixel is used only if (gx, gy) != (0, 0) and
 *        4 * (gx * wx + gy * wy)^2 >= 3 * (gx^2 + gy^2) * (wx^2 + wy^2),  (wx, wy) = (2x - x2, 2y - y2)
 *      -- gradients within 30 degrees of the radius; |wx|, |wy| <= 2057 and |gx|, |gy| <= 32768, so |gx * wx + gy * wy| <
 *      2^27.1, the left side is below 2^56.2 and the right below 3 * 2^31 * 2^23.1 < 2^55.7.  With REFINED_ONLY a pixel is
 *      used only if refined.  n = the used pixels.
 *   4. Moments, relative to the Hough circle: u = x_q8 - 128 * x2, v = y_q8 - 128 * y2, z = u^2 + v^2 - (256 * radius)^2.
 *      n, Su, Sv, Sz, Suu, Suv, Svv, Suz, Svz exactly (Suz, Svz in 128 bits, see the limits).  The Kasa fit z ~ a * u +
 *      b * v + c in a form whose numbers stay small because the points lie near the Hough circle.  Centred, exact (128 bits):
 *      A = n * Suu - Su^2, B = n * Suv - Su * Sv, C = n * Svv - Sv^2, P = n * Suz - Su * Sz, Q = n * Svz - Sv * Sz.
 *   5. Centre.  [A B; B C] * (a, b) = (P, Q); the centre moves by (a / 2, b / 2) in 1/256 px, i.e. by 128 * a in 1/65536 px.
 *      s = max(0, bitlength(max(A, C, |B|)) - 31); a' = A >> s, b' = B >> s, c' = C >> s (arithmetic shift: floor);
 *      det' = a' * c' - b'^2 (|.| < 2^62).  P and Q are NOT shifted (128-bit products carry them).
 *      Na = P * c' - Q * b', Nb = Q * a' - P * b'; e = 7 - s; for N in (Na, Nb):
 *        X = |N| * 2^max(e, 0), Y = det' * 2^max(-e, 0), q = floor((2 * X + Y) / (2 * Y)), the move = sgn(N) * q
 *      -- N * 2^e / det' to nearest, halves away from zero.  q <= limit is decided first, by 2 * X < Y * (2 * limit + 1) with
 *      limit = 65536 * (band + 2) < 2^19; the quotient then takes twenty steps of restoring division (compare, subtract,
 *      shift) on 128-bit values: the device has no 128-bit division and needs none.
 *      DEGENERATE iff n < 3, or det' <= 0, or either q > limit (the centre would move by more than band + 2 pixels).
 *      cx_q16 = 32768 * x2 + move_x, cy_q16 likewise.
 *      Error against the exact rational solution (a, b) of the unshifted system: the quotient is exact for the SHIFTED
 *      system, so with s = 0 the move is 128 * a rounded once.  With s > 0 each of a', b', c' is low by less than 1, and
 *        |move_x - 128 * a| <= 1/2 + 128 * (c' + |b'|) * (|a| + |b|) / det',
 *        |move_y - 128 * b| <= 1/2 + 128 * (a' + |b'|) * (|a| + |b|) / det'
 *      (x' - x = M'^-1 * E * x for the shifted matrix M' = M / 2^s - E, 0 <= E < 1 entrywise; M'^-1 = adj(M') / det').  For a
 *      full circle a' ~ c' ~ 2^30, b' ~ 0, det' ~ 2^60 and |a| + |b| < 2^12.6: the second term is below 2^-10.
 *   6. Radius and residuals, a pass over the used pixels: U = 256 * u - move_x, V = 256 * v - move_y (the point against the
 *      fitted centre in 1/65536 px), rho_q16 = isqrt(U^2 + V^2), the exact floor; e = rho_q16 - 65536 * radius;
 *      r_q16 = 65536 * radius + rdiv(sum of e, n), rdiv as in the line fits: the mean distance, the least-squares radius
 *      for the fitted centre.  d_q8 = (rho_q16 - r_q16 + 128) >> 8 (arithmetic shift).
 *   7. Trim, if trim_q8 > 0 and the first fit is not degenerate: the used set becomes the pixels of step 3 with
 *      |d_q8| <= trim_q8 against the first fit, and steps 4 to 6 run once more on that set.  One refit, never more.  If the
 *      trimmed set is degenerate, the record is the first fit's with CANNY_HIP_CIRCLE_FIT_TRIM_FAILED set.
 *   8. Statistics over the final used set against the final fit: n, Sdd = the sum of d_q8^2 (unsigned 64 bits), maxd =
 *      max |d_q8|, and sectors: bit k is set iff a used pixel lies in angular sector k around the fitted centre, with
 *      (dx, dy) = (U, V).  The plane is cut by the lines dy = 0, dx = 0, |dx| = |dy|, |dx| = 2 |dy|, |dy| = 2 |dx| into 16
 *      sectors, numbered from the +x axis towards the +y axis (clockwise on the screen, y pointing down): quadrant 0 is dx > 0,
 *      dy >= 0 with (p, q) = (dx, dy); quadrant 1 is dx <= 0, dy > 0 with (p, q) = (dy, -dx); quadrant 2 is dx < 0, dy <= 0
 *      with (p, q) = (-dx, -dy); quadrant 3 is dx >= 0, dy < 0 with (p, q) = (-dy, dx); k = 4 * quadrant + (2q >= p) +
 *      (q >= p) + (q >= 2p).  A pixel ON a boundary line belongs to the sector that STARTS there in this order; (0, 0)
 *      belongs to sector 0.  Sixteen bits set: a full circle; a run of few: an arc.
 *   9. Record: CANNY_HIP_CIRCLE_FIT_INTS = 8 32-bit words, 32 bytes:
 *        words 0-2: cx_q16, cy_q16, r_q16 (1/65536 px)      word 3: n
 *        word 4: maxd in bits 0-23, CANNY_HIP_CIRCLE_FIT_TRIM_FAILED (bit 27), _DEGENERATE (bit 28), _INVALID (bit 31)
 *        word 5: sectors in bits 0-15                        words 6-7: Sdd, low word first
 *      The caller's RMS distance is sqrt(Sdd / n) / 256 px.  A DEGENERATE record carries the Hough circle -- words 0-2 =
 *      32768 * x2, 32768 * y2, 65536 * radius -- then n; its words 5-7 and maxd are zero.
 *      The fit of circle slot f * centres_max + j goes to fit slot f * centres_max + j, for j < counts[f]; later slots are
 *      not touched.
 * Limits: max(height, width) <= CANNY_HIP_CIRCLE_FIT_MAX_AXIS = 16384 and band <= CANNY_HIP_CIRCLE_FIT_MAX_BAND = 4, else
 *   CANNY_HIP_ERR_UNSUPPORTED with nothing written; frames under 2 x 2: CANNY_HIP_ERR_INVALID, as for the edgels.  Widths:
 *     |u|, |v| <= 128 * (2 * 1028 + 1) + 128 < 2^18.01   (a pixel of the band against the centre, |t_q8| <= 128)
 *     n < 2^17           (the band is at most 9 pixels wide: fewer than 2 pi * 1029 * 10.5 < 2^16.1 lattice points)
 *     |z| < 2^29.5       (|rho - 256 * radius| <= 256 * 4.5 + 182, rho + 256 * radius < 2^19.01)
 *     |Su|, |Sv| < 2^35.1; |Sz| < 2^46.5; Suu, Svv, |Suv| < 2^53.1: 64 bits.
 *     |Suz|, |Svz| < 2^17 * 2^18.01 * 2^29.5 = 2^64.6: NOT 64 bits.  A lane of the kernel sums fewer than 2^15 products, each
 *       below 2^47.6, in 64 bits (16 queued pixels, or one 64-pixel word per turn of its rows' trips when the queue is
 *       full); across lanes the sums are carried as a high and a low half and joined in 128 bits.
 *     A, C, |B| < 2^70.1; |P|, |Q| < 2^82.6; a', c', |b'| < 2^31; |Na|, |Nb| < 2^114.6; e in -33 .. 7; X < 2^121.6, 2 X + Y <
 *       2^122.7; Y < 2^95, Y * (2 * limit + 1) < 2^115, 2 Y * 2^19 < 2^115: signed 128 bits throughout.
 *     |U|, |V| < 2^26.1 (the move is at most 2^18.6), U^2 + V^2 < 2^53.2: the root's argument is far below 2^63.
 *     |e| < 2^20; |sum of e| < 2^37; |d_q8| < 2^13, which fits the 24 bits of maxd; Sdd < 2^43.
 * The part is timed by canny_hip_circle_fits_profile_get (CANNY_HIP_CIRCLE_FIT_PART_FIT); with "profile_stage_mask" it goes
 * by bit 30 together with the polygon, edgel and line-fit parts.
 * Not covered -- follow-ups: Pratt / Taubin weighting, ellipses, several refits, colour / automatic-threshold /
 * batch-pipeline / sharder forms. */
#define CANNY_HIP_CIRCLE_FIT_INTS 8
#define CANNY_HIP_CIRCLE_FIT_GATE 1
#define CANNY_HIP_CIRCLE_FIT_REFINED_ONLY 2
#define CANNY_HIP_CIRCLE_FIT_MAXD_MASK 0x00ffffffu
#define CANNY_HIP_CIRCLE_FIT_TRIM_FAILED 0x08000000u
#define CANNY_HIP_CIRCLE_FIT_DEGENERATE 0x10000000u
#define CANNY_HIP_CIRCLE_FIT_INVALID 0x80000000u
#define CANNY_HIP_CIRCLE_FIT_MAX_AXIS 16384
#define CANNY_HIP_CIRCLE_FIT_MAX_BAND 4
#define CANNY_HIP_CIRCLE_FIT_MOMENT_WORDS 12
enum canny_hip_circle_fit_part {
    CANNY_HIP_CIRCLE_FIT_PART_FIT = 0, /* the one kernel: row walk, queue, edgels, the fits and the statistics */
    CANNY_HIP_CIRCLE_FIT_PARTS = 1
};
/* Host-only, needs no device: the rule in plain C++ on ONE host frame.  bits: the edge map in the layout of
 * canny_hip_dev_canny_bits; plane: height x width bytes if plane_is_u8 else shorts; circles: n_circles records of 6 ints;
 * fits receives n_circles records of 8 ints. */
int canny_hip_circle_fits_from_plane(const unsigned char *bits, const void *plane, int plane_is_u8, int height, int width,
                                     const int *circles, int n_circles, int band, int trim_q8, int options, int *fits);
/* Device bit maps (layout of canny_hip_dev_canny_bits, any byte alignment; the padding bits of a row are ignored, whatever
 * they hold), a device plane (bytes if plane_is_u8 else shorts, n_frames contiguous
 * planes) and the circle records and counts an earlier call left on the device (or the caller made: this is where INVALID
 * records come from).  d_plane == NULL means the smoothed plane the last canny_hip_dev_canny-family call on this context
 * left, under the rule of canny_hip_dev_edgels_at: CANNY_HIP_ERR_INVALID, nothing queued, if no such call ran or its shape
 * differs.  d_fits: n_frames * centres_max * 8 ints, 16-byte aligned, mandatory.  Asynchronous. */
int canny_hip_dev_circle_fits_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, const void *d_plane, int plane_is_u8,
                                   int n_frames, int height, int width, const int *d_circles, const int *d_counts,
                                   int centres_max, int band, int trim_q8, int options, int *d_fits);
/* canny_hip_dev_canny_hough_circles unchanged, then the fits queued behind it on the same stream, read from the converged
 * strong bit-plane and the smoothed plane that call left on the context.  d_circles and d_counts may be NULL (they then
 * live in a context workspace); d_fits is mandatory; everything else as there.  max_val > 255: all counts are 0 and no fit is
 * written. */
int canny_hip_dev_canny_hough_circle_fits(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                          int max_val, int height, int width, int n_frames, short *d_edges, int min_radius,
                                          int max_radius, int cell_shift, int threshold, int support_threshold,
                                          int min_dist, int centres_max, int *d_circles, int *d_counts,
                                          int *d_centre_counts, int *d_accum, int band, int trim_q8, int options,
                                          int *d_fits);
/* Host buffers, synchronous, in the pattern of canny_hip_canny_hough_circles: the counts come down first, then only the
 * filled slots of circles and fits.  circles and centre_counts may be NULL; counts and fits are mandatory. */
int canny_hip_canny_hough_circle_fits(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                                      int max_val, int height, int width, int min_radius, int max_radius, int cell_shift,
                                      int threshold, int support_threshold, int min_dist, int centres_max, int band,
                                      int trim_q8, int options, int *circles, int *counts, int *centre_counts, int *fits);
/* Test hook: the device finishing function (steps 4 and 5) on n_sets moment sets of CANNY_HIP_CIRCLE_FIT_MOMENT_WORDS = 12
 * long longs (n, Su, Sv, Sz, Suu, Suv, Svv, Suz low, Suz high, Svz low, Svz high, band; Suz and Svz two's-complement 128-bit
 * values), the sums within the limits above and band in 0 .. 4; d_out receives 4 ints per set: move_x, move_y (both 0 if
 * degenerate), n, then CANNY_HIP_CIRCLE_FIT_DEGENERATE or 0.  Asynchronous. */
int canny_hip_dev_circle_fits_arith(canny_hip_ctx *ctx, const long long *d_moments, size_t n_sets, int *d_out);
/* Host-only, the same hook on the plain C++ restatement (host arrays). */
int canny_hip_circle_fits_finish(const long long *moments, size_t n_sets, int *out);
/* Host-only: how many pixels of one record the fit kernel keeps in its LDS queue; a record with more pixels in its band is
 * finished by recomputing the rest, with the same bytes.  For the test that exceeds it on purpose. */
int canny_hip_circle_fits_queue_capacity(void);

/* ---- connected components ------------------------------------------------------------------------------------------------
 * Eight-connected component labelling of the finished edge map, per frame of a batch, on the GPU, queued behind the detector
 * on the same stream with no host round trip: the grouping of edge pixels into curves that contour following starts from, and
 * the "drop the short fragments" filter that is usually applied first.  THE RULE, for frame f with
 * edge map E_f (the map canny_hip_canny returns for that frame, bit for bit):
 *   Components: the set pixels (E_f[r][c] != 0) are partitioned by 8-connectivity (two set pixels whose rows and columns both
 *     differ by at most 1 belong together).  A component has area = its pixel count and first = its smallest index r*width+c.
 *   Filter: components with area >= min_area are KEPT; min_area <= 1 keeps all of them.
 *   Numbering: kept components are numbered 1 .. K_f by ascending first.  With min_area <= 1 this is
 *     scipy.ndimage.label(mask, structure=np.ones((3, 3))); up to the numbering it is cv::connectedComponents(mask, 8).
 *   labels (int, [n][height][width]): the component's number on its pixels; 0 on background and on dropped components.
 *     Every element is written.
 *   kept_u8 (unsigned char, layout of canny_hip_dev_canny_u8): 255 where labels != 0, else 0.  Every element is written.
 *   stats: CANNY_HIP_CC_STATS = 6 ints per kept component, CANNY_HIP_CC_STAT_LEFT, _TOP, _WIDTH, _HEIGHT, _AREA (the bounding
 *     box and pixel count: the column order of cv::connectedComponentsWithStats, without its background row), then
 *     CANNY_HIP_CC_STAT_FIRST.
 *   CSR over the batch, as for the point lists: offsets[0 .. n_frames] (unsigned long long), offsets[0] = 0,
 *     offsets[f+1] - offsets[f] = K_f -- always the TRUE counts; the record of label k of frame f is record
 *     offsets[f] + k - 1 of stats.  `capacity` counts RECORDS and bounds the writes, never the counts: records at positions
 *     >= capacity are not written, nothing is written at or past stats + 6 * capacity, and every record below it is exact.
 *   offsets is mandatory; any of labels, kept_u8, stats may be NULL, and what the others receive does not depend on that.
 *     stats == NULL with capacity > 0 is CANNY_HIP_ERR_INVALID (stats == NULL, capacity == 0: counts only).
 *   The result follows the MAP, not the plane it is derived from: max_val > 255 empties every map (see the point lists), so
 *     all offsets are 0 and labels / kept_u8 all zero.
 *   Statuses are those of canny_hip_dev_canny for the same arguments, which runs first; on a status other than OK nothing
 *     is written.  Pixel indices are 32-bit: a frame of 2^31 pixels or more is CANNY_HIP_ERR_UNSUPPORTED, as everywhere.
 *   The output is the same bytes on every run.  Integer atomics (min, max, add) decide WHEN two trees of the union-find are
 *     merged, never what comes out: partition, first, area and box are order-independent, and the numbering is a prefix sum
 *     in raster order, not a counter.
 * Memory: with labels == NULL a context workspace of 4 bytes per pixel of the batch holds the union-find's parent array (it
 *   is touched per run of set pixels, not per pixel); with labels given that array lives in the label plane itself.
 * The four parts are timed by canny_hip_components_profile_get (CANNY_HIP_CC_PART_*); with "profile_stage_mask" they are
 *   bits 13 .. 16 (the Hough parts are bits 10 .. 12).
 * Not covered -- follow-ups: 4-connectivity, centroids, the three-stream batch pipeline, the multi-GPU sharder, colour and
 * per-frame / automatic-threshold variants.  (Contour chains: the next section.) */
#define CANNY_HIP_CC_STATS 6
enum canny_hip_cc_stat {
    CANNY_HIP_CC_STAT_LEFT = 0,
    CANNY_HIP_CC_STAT_TOP = 1,
    CANNY_HIP_CC_STAT_WIDTH = 2,
    CANNY_HIP_CC_STAT_HEIGHT = 3,
    CANNY_HIP_CC_STAT_AREA = 4,
    CANNY_HIP_CC_STAT_FIRST = 5
};
enum canny_hip_cc_part {
    CANNY_HIP_CC_PART_LINK = 0,     /* parent array set up, touching runs united (union-find, atomicMin) */
    CANNY_HIP_CC_PART_RESOLVE = 1,  /* every run finds its root; areas summed onto the roots */
    CANNY_HIP_CC_PART_NUMBER = 2,   /* kept roots counted per row, scanned, numbered; records and boxes written */
    CANNY_HIP_CC_PART_WRITE = 3,    /* labels and kept_u8 stored */
    CANNY_HIP_CC_PARTS = 4
};
/* Device buffers, asynchronous; completion contract and d_edges as canny_hip_dev_canny_points.  canny_hip_dev_canny itself
 * queues exactly what it queues on its own; the labelling reads the converged hysteresis bit-plane behind it. */
int canny_hip_dev_canny_components(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                   int height, int width, int n_frames, short *d_edges, int min_area, int *d_labels,
                                   unsigned char *d_kept_u8, int *d_stats, unsigned long long capacity,
                                   unsigned long long *d_offsets);
/* The labelling alone, on device bit maps in the layout of canny_hip_dev_canny_bits (rows MSB-first, padded to bytes; any
 * byte alignment; the padding bits of a row are ignored, whatever they hold).  Asynchronous. */
int canny_hip_dev_components_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                  int min_area, int *d_labels, unsigned char *d_kept_u8, int *d_stats,
                                  unsigned long long capacity, unsigned long long *d_offsets);
/* Host buffers, synchronous: upload, canny, labelling; the offsets come down first, then min(offsets[n_frames], capacity)
 * records and only the planes that were asked for. */
int canny_hip_canny_components(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                               int max_val, int height, int width, int min_area, int *labels, unsigned char *kept_u8,
                               int *stats, unsigned long long capacity, unsigned long long *offsets);
/* Host-only, needs no device: the same rule on ONE host bit map, in plain C++ (two passes, union-find) -- what a caller of
 * canny_hip_canny_batch_bits runs on the maps it received.  labels (height * width ints) and stats may be NULL; *count
 * receives the true number of kept components. */
int canny_hip_components_from_bits(const unsigned char *bits, int height, int width, int min_area, int *labels,
                                   int *stats, unsigned long long capacity, unsigned long long *count);

/* ---- outer contour chains ------------------------------------------------------------------------------------------------
 * For every kept component of the finished edge map its outer border as an ORDERED list of pixels, per frame of a batch, on
 * the GPU, queued behind the detector on the same stream with no host round trip: what curve fitting, polygon approximation,
 * arc-length measures, shape descriptors and vector export start from (polygon approximation: the section after this one) --
 * the use of
 * cv::findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) after cv::Canny.  (The same curves; no claim is made that the points
 * come in the order OpenCV lists them.)  THE RULE, for frame f with edge map E_f (the map
 * canny_hip_canny returns for that frame, bit for bit):
 *   Components, the min_area filter and the numbering are exactly those of the connected components above.  For each kept
 *     component the CHAIN is its outer border, followed as in Suzuki & Abe's border following restricted to outer borders,
 *     with 8-connectivity, starting at the component's first pixel.
 *   Directions are numbered clockwise on the displayed image, as (row, column) steps: 0 = E (0,+1), 1 = SE (+1,+1),
 *     2 = S (+1,0), 3 = SW (+1,-1), 4 = W (0,-1), 5 = NW (-1,-1), 6 = N (-1,0), 7 = NE (-1,+1).  Pixels outside the frame
 *     are unset.
 *   1. p0 = first.  Examine p0's neighbours clockwise after W, in directions 5, 6, 7, 0, 1, 2, 3.  The first set one is q1,
 *      in direction d_last.  If there is none, the chain is [p0].
 *   2. Otherwise cur = p0 and s = (d_last - 1) & 7.  Repeat: examine cur's neighbours counter-clockwise in directions
 *      s, s - 1, ... (mod 8, all eight); the first set one is nxt, in direction d.  If nxt == p0 and cur == q1, stop.
 *      Otherwise append nxt, then cur = nxt and s = (d + 3) & 7.
 *   3. The chain is p0 followed by the appended pixels, as indices r * width + c (the point lists' convention); p0 is not
 *      repeated at the end.  Consecutive chain pixels, cyclically, are distinct 8-neighbours; a one-pixel-wide curve is
 *      walked out and back, so a pixel may occur more than once.  As a set the chain is the component's pixels that have a
 *      4-neighbour in the background region outside the component.
 *   A walk is a sequence of states (cur, s) that ends before a state recurs, so a chain has at most 8 * area points; the
 *     device walks are capped at 8 * area steps, which no map reaches.
 *   Outputs, CSR on two levels (all offsets unsigned long long):
 *     offsets[0 .. n_frames]: the record CSR over the batch, identical to what the components calls return for the same
 *       min_area -- always the TRUE counts.  K = offsets[n_frames].
 *     point_offsets[0 .. n_frames]: the CSR of chain POINTS per frame -- always the TRUE counts.  A counts-only call
 *       (capacity = 0, point_capacity = 0, the other pointers NULL) sizes both buffers.
 *     chain_offsets[j] for j = 0 .. min(K, capacity) (so capacity + 1 entries at most): the number of chain points of
 *       records 0 .. j - 1, true prefix sums over the whole batch.  Record j's chain is
 *       points[chain_offsets[j] .. chain_offsets[j + 1]).  Entries past min(K, capacity) are not written.
 *       point_offsets[f] == chain_offsets[offsets[f]] wherever that entry exists.
 *     points (int): position q is written iff q < point_capacity and it belongs to a record < capacity: the prefix that fits
 *       is exact, a chain may be cut, nothing is written at or past points + point_capacity.
 *     stats (optional, may be NULL at any capacity): the 6-int records of the connected components, bounded by capacity.
 *   offsets and point_offsets are mandatory.  points == NULL with point_capacity > 0 and chain_offsets == NULL with
 *     capacity > 0 are CANNY_HIP_ERR_INVALID.
 *   The result follows the MAP: max_val > 255 empties every map, so all offsets and point_offsets are 0 (and
 *     chain_offsets[0] = 0 if given).
 *   Limits: height * width <= 2^28 (the chain points of a frame are summed in 32 bits), beyond that
 *     CANNY_HIP_ERR_UNSUPPORTED before anything is queued.  Otherwise the statuses are those of canny_hip_dev_canny for the
 *     same arguments, which runs first; on a status other than OK nothing is written.
 *   The output is the same bytes on every run: lengths and positions are prefix sums in raster order of the first pixels,
 *     every point is stored once by the one thread that walks its chain, and the launches depend on the shapes and on which
 *     outputs were asked for, never on the data.
 * Memory: a context workspace of 4 bytes per pixel of the batch (the union-find's parent array, shared with the components
 *   calls) and 4 bytes per image row.
 * Cost: a chain is walked by ONE thread, twice (lengths, then points), so a call takes as long as its longest chain; see
 *   DESIGN.md section 17 for the measured time per step.
 * The four parts are timed by canny_hip_contours_profile_get (CANNY_HIP_CONTOUR_PART_*); with "profile_stage_mask" they are
 *   bits 22 .. 25.
 * Not covered -- follow-ups: hole borders and the hierarchy, CHAIN_APPROX_SIMPLE as its own call, 4-connectivity,
 * sub-pixel positions, parallel ranking of long chains, the three-stream batch pipeline, the multi-GPU sharder, colour and
 * per-frame / automatic-threshold variants. */
enum canny_hip_contour_part {
    CANNY_HIP_CONTOUR_PART_LABEL = 0,  /* union-find on runs, roots and areas, kept roots counted and scanned: offsets */
    CANNY_HIP_CONTOUR_PART_COUNT = 1,  /* first walk: chain lengths, scanned and placed: point_offsets, chain_offsets */
    CANNY_HIP_CONTOUR_PART_WRITE = 2,  /* second walk: points stored */
    CANNY_HIP_CONTOUR_PART_STATS = 3,  /* the components' records, when stats was asked for */
    CANNY_HIP_CONTOUR_PARTS = 4
};
/* Device buffers, asynchronous; completion contract and d_edges as canny_hip_dev_canny_points.  canny_hip_dev_canny itself
 * queues exactly what it queues on its own; the walks read the converged hysteresis bit-plane behind it. */
int canny_hip_dev_canny_contours(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                 int height, int width, int n_frames, short *d_edges, int min_area, int *d_stats,
                                 unsigned long long capacity, unsigned long long *d_offsets,
                                 unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                 unsigned long long *d_point_offsets);
/* The chains alone, on device bit maps in the layout of canny_hip_dev_canny_bits (rows MSB-first, padded to bytes; any
 * byte alignment; the padding bits of a row are ignored, whatever they hold).  Asynchronous. */
int canny_hip_dev_contours_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                int min_area, int *d_stats, unsigned long long capacity, unsigned long long *d_offsets,
                                unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                unsigned long long *d_point_offsets);
/* Host buffers, synchronous: upload, canny, chains; offsets and point_offsets come down first, then what fits:
 * min(K, capacity) + 1 chain offsets, as many records, and the points below min(chain_offsets[min(K, capacity)],
 * point_capacity). */
int canny_hip_canny_contours(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                             int max_val, int height, int width, int min_area, int *stats, unsigned long long capacity,
                             unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                             unsigned long long point_capacity, unsigned long long *point_offsets);
/* Host-only, needs no device: the same rule on ONE host bit map, in plain C++.  *count receives the true number of kept
 * components, *point_count the true number of chain points; both are mandatory. */
int canny_hip_contours_from_bits(const unsigned char *bits, int height, int width, int min_area, int *stats,
                                 unsigned long long capacity, unsigned long long *count,
                                 unsigned long long *chain_offsets, int *points, unsigned long long point_capacity,
                                 unsigned long long *point_count);

/* ---- polygon approximation of the contour chains ---------------------------------------------------------------------------
 * For every stored chain of a contours call the few vertices that describe it, on the GPU, queued behind the chains on the
 * same stream: the use of cv::approxPolyDP(c, eps * cv::arcLength(c, true), true) after cv::findContours, and what "four
 * vertices, convex, large enough: a rectangle" is decided on.  A chain is every border pixel in order; a polygon is a
 * handful of vertices, the only form of the contours that is cheap to bring to the host.  Everything is integers.
 * THE RULE, for one stored chain P_0 .. P_{n-1}.  Points are pixel indices r * width + c, read as
 * (x, y) = (c, r); the chain is closed, P_n means P_0.  The parameters of a call: epsilon_q8 (unsigned), an absolute
 * tolerance in 1/256 pixel, and ratio_q16 (unsigned, < 65536), a tolerance relative to the chain's own length in 1/65536.
 * Both may be given; they add.
 *   1. Length.  length_q8 = 256 * (number of axis steps) + 362 * (number of diagonal steps) over the n cyclic steps
 *      P_i -> P_{i+1}: a step that changes both coordinates is diagonal, one that changes exactly one is an axis step, a
 *      step between equal points (n == 1) counts nothing, so the length of a one-point chain is 0.  362 / 256 stands for
 *      sqrt(2) and is part of the rule: length_q8 / 256 is cv::arcLength(chain, true) to within 0.02 %.  64-bit arithmetic.
 *   2. Tolerance.  eps = min(epsilon_q8 + ((ratio_q16 * length_q8) >> 16), 2^24).
 *   3. Anchors.  n == 1: the polygon is [P_0].  Otherwise k is the smallest i that maximises |P_i - P_0|^2; positions 0 and
 *      k are vertices.
 *   4. Simplify the two open runs (0, k) and (k, n).  Simplifying (a, b) with b - a >= 2: for a < i < b let
 *      c_i = |cross(P_b - P_a, P_i - P_a)|; m is the smallest i that maximises c_i.  If c_m^2 * 2^16 > eps^2 * |P_b - P_a|^2,
 *      compared exactly (128 bits), position m is a vertex and (a, m) and (m, b) are simplified in turn; otherwise nothing
 *      between a and b is a vertex.  The two ends of every run are different pixels (the anchors differ, and a kept m has
 *      c_m > 0), so no zero-length base occurs and there is no special case.
 *   5. The polygon is the list of vertex positions in chain order, returned as the pixel indices P_i.  eps = 0 drops
 *      exactly the collinear points; a one-pixel-wide curve, which the chain walks out and back, comes down to its turning
 *      points.
 *   6. Measures per record, four long long: CANNY_HIP_POLYGON_VERTICES the true count V; _LENGTH_Q8; _AREA2 =
 *      |sum of x_i * y_{i+1} - x_{i+1} * y_i| over the polygon's vertices, cyclically -- twice cv::contourArea of the
 *      polygon; _CONVEX = 1 iff V >= 3 and the turns cross(v_{i+1} - v_i, v_{i+2} - v_{i+1}) are all >= 0 or all <= 0 with
 *      at least one of them non-zero, otherwise 0.
 *   Which chains: the stage reads chains where a contours call stored them, so it handles the records
 *     j < R = min(K, capacity).  A record is COMPLETE iff chain_offsets[j + 1] <= point_capacity.  An incomplete record --
 *     its chain was cut by the caller's buffer -- has no vertices and the measures (-1, 0, 0, 0).
 *   Outputs:
 *     vertex_offsets[0 .. R] (unsigned long long, capacity + 1 entries at most; mandatory): the true prefix sums of V over
 *       the records, incomplete records counting 0.  Entries past R are not written.
 *     vertices (int): position q is written iff q < vertex_capacity: the prefix that fits is exact, a polygon may be cut,
 *       nothing is written at or past vertices + vertex_capacity.  NULL is allowed with vertex_capacity == 0 only.
 *     measures (optional, long long [R][4]); what the other outputs receive does not depend on its presence.
 *   Arguments: chain_offsets, offsets and vertex_offsets are mandatory (chain_offsets and vertex_offsets have capacity + 1
 *     entries, so they exist at capacity 0 too); points may be NULL with point_capacity == 0 only; ratio_q16 >= 65536 and
 *     n_frames < 1 are CANNY_HIP_ERR_INVALID.  A height or width above 32768 is CANNY_HIP_ERR_UNSUPPORTED before anything is
 *     queued (every cross product stays below 2^31).  All other limits and statuses are those of the contours calls, which
 *     run first and unchanged; on a status other than OK nothing is written.  An empty map (max_val > 255 included) gives
 *     all zeros: vertex_offsets[0] = 0 and nothing else.
 *   The output is the same bytes on every run: there are no atomics, every element is stored once by one wave, and the
 *     launches depend on the shapes, the capacities and on which outputs were asked for, never on the data.
 * Memory: a context workspace of one byte per point slot (point_capacity) for the vertex flags of chains longer than 64
 *   points, 8 bytes per record slot (capacity) for the vertex masks of the others, and 8 bytes per 2048 record slots.
 * Cost: a chain is simplified by ONE wave; chains of at most 64 points, the bulk of an edge map, stay in registers.  See
 *   DESIGN.md section 19 for the measured times, the long-chain tail included.
 * The three parts are timed by canny_hip_polygons_profile_get (CANNY_HIP_POLYGON_PART_*); with "profile_stage_mask" the
 *   three go by bit 30 together, the last bit a non-negative int option carries.
 * Not covered -- follow-ups: hole borders, open-curve mode (closed = false), CHAIN_APPROX_SIMPLE as its own call, long
 * chains split over a workgroup, the three-stream batch pipeline, the multi-GPU sharder, colour and per-frame /
 * automatic-threshold variants. */
#define CANNY_HIP_POLYGON_MEASURES 4
enum canny_hip_polygon_measure {
    CANNY_HIP_POLYGON_VERTICES = 0,
    CANNY_HIP_POLYGON_LENGTH_Q8 = 1,
    CANNY_HIP_POLYGON_AREA2 = 2,
    CANNY_HIP_POLYGON_CONVEX = 3
};
enum canny_hip_polygon_part {
    CANNY_HIP_POLYGON_PART_SIMPLIFY = 0,  /* one wave per chain: length, anchors, the descent; vertex counts */
    CANNY_HIP_POLYGON_PART_SCAN = 1,      /* prefix sums of the counts: vertex_offsets */
    CANNY_HIP_POLYGON_PART_EMIT = 2,      /* vertices stored in chain order; area2 and convex */
    CANNY_HIP_POLYGON_PARTS = 3
};
/* The stage alone, on chains already on the device: d_offsets, d_chain_offsets and d_points are what a contours call with
 * the same n_frames, capacity and point_capacity left.  Asynchronous, on the context's stream. */
int canny_hip_dev_polygons_chains(canny_hip_ctx *ctx, const unsigned long long *d_offsets, int n_frames,
                                  unsigned long long capacity, const unsigned long long *d_chain_offsets,
                                  const int *d_points, unsigned long long point_capacity, int width, int height,
                                  unsigned epsilon_q8, unsigned ratio_q16, unsigned long long *d_vertex_offsets,
                                  int *d_vertices, unsigned long long vertex_capacity, long long *d_measures);
/* canny_hip_dev_canny_contours / canny_hip_dev_contours_bits, unchanged, then the stage on what they stored. */
int canny_hip_dev_canny_polygons(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                 int height, int width, int n_frames, short *d_edges, int min_area, int *d_stats,
                                 unsigned long long capacity, unsigned long long *d_offsets,
                                 unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                 unsigned long long *d_point_offsets, unsigned epsilon_q8, unsigned ratio_q16,
                                 unsigned long long *d_vertex_offsets, int *d_vertices, unsigned long long vertex_capacity,
                                 long long *d_measures);
int canny_hip_dev_polygons_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                                int min_area, int *d_stats, unsigned long long capacity, unsigned long long *d_offsets,
                                unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                                unsigned long long *d_point_offsets, unsigned epsilon_q8, unsigned ratio_q16,
                                unsigned long long *d_vertex_offsets, int *d_vertices, unsigned long long vertex_capacity,
                                long long *d_measures);
/* Host buffers, synchronous: upload, canny, chains, polygons.  Everything canny_hip_canny_contours returns comes down, plus
 * min(K, capacity) + 1 vertex offsets, as many measures, and the vertices below min(vertex_offsets[min(K, capacity)],
 * vertex_capacity).  points may be NULL here at any point_capacity: the chains then stay in a device buffer of
 * point_capacity ints and only the polygons cross to the host -- the point of the feature.  chain_offsets, stats and
 * measures may be NULL. */
int canny_hip_canny_polygons(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                             int max_val, int height, int width, int min_area, int *stats, unsigned long long capacity,
                             unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                             unsigned long long point_capacity, unsigned long long *point_offsets, unsigned epsilon_q8,
                             unsigned ratio_q16, unsigned long long *vertex_offsets, int *vertices,
                             unsigned long long vertex_capacity, long long *measures);
/* Host-only, needs no device: the same rule in plain C++ on n_records chains in host memory (what a caller of
 * canny_hip_canny_contours or canny_hip_contours_from_bits holds).  vertex_offsets has n_records + 1 entries. */
int canny_hip_polygons_from_chains(const unsigned long long *chain_offsets, const int *points,
                                   unsigned long long n_records, unsigned long long point_capacity, int width, int height,
                                   unsigned epsilon_q8, unsigned ratio_q16, unsigned long long *vertex_offsets,
                                   int *vertices, unsigned long long vertex_capacity, long long *measures);

/* ---- contour shape measures: moments, convex hull, minimum-area rectangle ---------------------------------------------------
 * For every stored chain of a contours call what a caller of cv::findContours reaches for next, on the GPU, queued behind the
 * chains on the same stream: the integers behind cv::moments (centroid, orientation), cv::convexHull (solidity) and
 * cv::minAreaRect (the oriented box: "a rotated rectangle / a bar / a part in a gripper"), 20 words and a handful of hull
 * vertices per contour instead of a download of the chains.  Everything is integers and exact.
 * THE RULE, for one stored chain P_0 .. P_{n-1}.  Points are pixel indices r * width + c, read as
 * (x, y) = (c, r); the chain is closed, P_n means P_0.  All moments are relative to the anchor P_0: u_i = x_i - x_0,
 * v_i = y_i - y_0.  Every sum below is taken in 64-bit two's-complement WRAPPING arithmetic and read back as signed: the
 * stored word is the true value whenever that fits, whatever the partial sums did in between, and it fits for every outer
 * border of a frame within the size limit (height, width < 32768).
 *   1. Polygon moments (Green's theorem; the integers behind cv::moments(contour)).  With a_i = u_i * v_{i+1} - u_{i+1} * v_i
 *      over the n cyclic steps:
 *        area2  = sum a_i   (signed: the sign is the walk's orientation; twice the area)
 *        m10_6  = sum a_i * (u_i + u_{i+1})                              m01_6 likewise in v   (6 * m10, 6 * m01)
 *        m20_12 = sum a_i * (u_i^2 + u_i * u_{i+1} + u_{i+1}^2)          m02_12 likewise in v  (12 * m20, 12 * m02)
 *        m11_24 = sum a_i * (2 u_i v_i + u_i v_{i+1} + u_{i+1} v_i + 2 u_{i+1} v_{i+1})         (24 * m11)
 *   2. Point sums over the n chain points: s10 = sum u, s01 = sum v, s20 = sum u^2, s11 = sum u * v, s02 = sum v^2.  A Canny
 *      map is mostly one-pixel curves that the border follower walks out and back; their area2 is 0, and these sums are what
 *      gives such a curve a centre and an axis.
 *   3. Convex hull of the chain's point set.  The vertices are the strictly extreme points (a point on a hull edge between
 *      two others is no vertex).  The order begins at the vertex with the smallest x, among those the smallest y, and
 *      continues so that every turn cross(H_{k+1} - H_k, H_{k+2} - H_{k+1}) > 0 with x to the right and y down.  The hull is
 *      stored as pixel indices; V_h is its true vertex count.  hull_area2 = sum x_k * y_{k+1} - x_{k+1} * y_k >= 0.
 *   4. Minimum-area rectangle with a side on a hull edge.  For edge k: d = H_{k+1} - H_k, len2 = |d|^2,
 *      along_i = dot(H_i - H_k, d), across_i = cross(d, H_i - H_k) (>= 0 by the orientation), E_k = max along - min along,
 *      N_k = max across; the rectangle's area is E_k * N_k / len2_k.  The chosen edge is the smallest k that minimises that
 *      area; two edges are compared exactly as E_k N_k len2_k' against E_k' N_k' len2_k (E * N < 2^63, len2 < 2^31: 128
 *      bits).  Stored: rect_edge = k, rect_along_min, rect_along_max, rect_across = N_k, rect_len2: the caller gets corners,
 *      size and angle from these and the two hull vertices H_k, H_{k+1} without any rounding by the library.  V_h = 2:
 *      rect_edge 0, along_min 0, along_max = len2, across 0.  V_h = 1: all zero.
 *   5. Measures per record, CANNY_HIP_SHAPE_WORDS = 20 long long, in the order of enum canny_hip_shape_measure.
 *   Which chains: as for the polygons, the records j < R = min(K, capacity); a record is COMPLETE iff
 *     chain_offsets[j + 1] <= point_capacity.  An incomplete record has hull_vertices = -1, 19 zeros and no hull vertices.
 *   Outputs:
 *     hull_offsets[0 .. R] (unsigned long long, capacity + 1 entries at most; mandatory): the true prefix sums of V_h,
 *       incomplete records counting 0.  Entries past R are not written.
 *     hull (int): position q is written iff q < hull_capacity: the prefix that fits is exact, nothing is written at or past
 *       hull + hull_capacity.  NULL is allowed with hull_capacity == 0 only.
 *     measures (optional, long long [R][20]); what the other outputs receive does not depend on which outputs are absent.
 *       hull_area2 and the rectangle come from the hull itself, not from what fitted into the caller's buffer.
 *   Arguments: as for the polygons calls without the tolerances.  A height or width of 32768 or more is
 *     CANNY_HIP_ERR_UNSUPPORTED before anything is queued.  On a status other than OK nothing is written.  An empty map
 *     (max_val > 255 included) gives hull_offsets[0] = 0 and nothing else.  The device calls expect what a contours call
 *     stores, closed 8-connected walks: a chain whose bounding box is wider than the chain is long, or that visits no point
 *     of some column of its box, is answered like an incomplete record (canny_hip_shapes_from_chains measures any chain).
 *   The output is the same bytes on every run: every output element is stored once by one wave; the only atomics are
 *     integer minima and maxima into a workspace, whose result does not depend on the order in which they land; the
 *     launches depend on the shapes, the capacities and on which outputs were asked for, never on the data.
 * Memory: a context workspace of 20 bytes per point slot (point_capacity): per column of a chain's bounding box the smallest
 *   and the largest y, two lists for the rounds of the hull, and the finished hull; plus 8 bytes per 2048 record slots.
 * Cost: a chain is measured by ONE wave.  See DESIGN.md section 27 for the measured times, the long-chain tail included.
 * The three parts are timed by canny_hip_shapes_profile_get (CANNY_HIP_SHAPE_PART_*); with "profile_stage_mask" they go by
 *   bit 30 like every part behind the polygons.
 * Not covered -- follow-ups: hole borders, convexity defects, ellipse fits, the minimum enclosing circle, Hu invariants
 * (floats the caller derives from these words), the three-stream batch pipeline, the multi-GPU sharder, colour and
 * per-frame / automatic-threshold variants, long chains split over a workgroup. */
#define CANNY_HIP_SHAPE_WORDS 20
enum canny_hip_shape_measure {
    CANNY_HIP_SHAPE_HULL_VERTICES = 0,
    CANNY_HIP_SHAPE_POINTS = 1,
    CANNY_HIP_SHAPE_ANCHOR = 2,
    CANNY_HIP_SHAPE_AREA2 = 3,
    CANNY_HIP_SHAPE_M10_6 = 4,
    CANNY_HIP_SHAPE_M01_6 = 5,
    CANNY_HIP_SHAPE_M20_12 = 6,
    CANNY_HIP_SHAPE_M11_24 = 7,
    CANNY_HIP_SHAPE_M02_12 = 8,
    CANNY_HIP_SHAPE_S10 = 9,
    CANNY_HIP_SHAPE_S01 = 10,
    CANNY_HIP_SHAPE_S20 = 11,
    CANNY_HIP_SHAPE_S11 = 12,
    CANNY_HIP_SHAPE_S02 = 13,
    CANNY_HIP_SHAPE_HULL_AREA2 = 14,
    CANNY_HIP_SHAPE_RECT_EDGE = 15,
    CANNY_HIP_SHAPE_RECT_ALONG_MIN = 16,
    CANNY_HIP_SHAPE_RECT_ALONG_MAX = 17,
    CANNY_HIP_SHAPE_RECT_ACROSS = 18,
    CANNY_HIP_SHAPE_RECT_LEN2 = 19
};
enum canny_hip_shape_part {
    CANNY_HIP_SHAPE_PART_MEASURE = 0,  /* one wave per chain: the eleven sums, the column extremes, the hull; hull counts */
    CANNY_HIP_SHAPE_PART_SCAN = 1,     /* prefix sums of the counts: hull_offsets */
    CANNY_HIP_SHAPE_PART_EMIT = 2,     /* hull vertices stored; hull_area2 and the rectangle */
    CANNY_HIP_SHAPE_PARTS = 3
};
/* The stage alone, on chains already on the device: d_offsets, d_chain_offsets and d_points are what a contours call with
 * the same n_frames, capacity and point_capacity left (a polygons call may have run on them in between).  Asynchronous, on
 * the context's stream. */
int canny_hip_dev_shapes_chains(canny_hip_ctx *ctx, const unsigned long long *d_offsets, int n_frames,
                                unsigned long long capacity, const unsigned long long *d_chain_offsets, const int *d_points,
                                unsigned long long point_capacity, int width, int height,
                                unsigned long long *d_hull_offsets, int *d_hull, unsigned long long hull_capacity,
                                long long *d_measures);
/* canny_hip_dev_canny_contours / canny_hip_dev_contours_bits, unchanged, then the stage on what they stored. */
int canny_hip_dev_canny_shapes(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, int min_area, int *d_stats,
                               unsigned long long capacity, unsigned long long *d_offsets,
                               unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                               unsigned long long *d_point_offsets, unsigned long long *d_hull_offsets, int *d_hull,
                               unsigned long long hull_capacity, long long *d_measures);
int canny_hip_dev_shapes_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                              int min_area, int *d_stats, unsigned long long capacity, unsigned long long *d_offsets,
                              unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                              unsigned long long *d_point_offsets, unsigned long long *d_hull_offsets, int *d_hull,
                              unsigned long long hull_capacity, long long *d_measures);
/* Host buffers, synchronous: upload, canny, chains, shapes.  Everything canny_hip_canny_contours returns comes down, plus
 * min(K, capacity) + 1 hull offsets, as many measures, and the hull vertices below min(hull_offsets[min(K, capacity)],
 * hull_capacity).  points may be NULL here at any point_capacity: the chains then stay in a device buffer of point_capacity
 * ints and only the shapes cross to the host.  chain_offsets, stats and measures may be NULL. */
int canny_hip_canny_shapes(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int min_area, int *stats, unsigned long long capacity,
                           unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                           unsigned long long point_capacity, unsigned long long *point_offsets,
                           unsigned long long *hull_offsets, int *hull, unsigned long long hull_capacity,
                           long long *measures);
/* Host-only, needs no device: the same rule in plain C++ on n_records chains in host memory.  hull_offsets has
 * n_records + 1 entries. */
int canny_hip_shapes_from_chains(const unsigned long long *chain_offsets, const int *points, unsigned long long n_records,
                                 unsigned long long point_capacity, int width, int height, unsigned long long *hull_offsets,
                                 int *hull, unsigned long long hull_capacity, long long *measures);

/* ---- edge curves: the edge map linked into ordered chains ------------------------------------------------------------------
 * Edge linking, per frame of a batch, on the GPU, queued behind the detector on the same stream with no host round trip:
 * every edge pixel is taken ONCE, in order along its curve; curves are split where they meet; open and closed curves are
 * told apart -- what curve fitting to the edges, skeleton graphs and vector export start from (the use of Kovesi's
 * edgelink after a Canny map).  A contour chain (the section above the polygons) is the border of a component and walks a
 * one-pixel curve out and back; a curve lists it once.  THE RULE, for frame f with edge map E_f
 * (the map canny_hip_canny returns for that frame, bit for bit).  It is all integers and purely a function of the map.
 *   Directions are those of the contour chains: 0 = E (0,+1), 1 = SE (+1,+1), 2 = S (+1,0), 3 = SW (+1,-1), 4 = W (0,-1),
 *     5 = NW (-1,-1), 6 = N (-1,0), 7 = NE (-1,+1), as (row, column) steps.  Pixels outside the frame are unset.  Frames
 *     never see each other.  index(p) = r * width + c.
 *   1. Links.  Two set 8-neighbours are LINKED if they are 4-neighbours; diagonal neighbours are linked only if neither of
 *      the two pixels 4-adjacent to both is set (a diagonal that a staircase corner already bridges is not a link).  As a
 *      byte operation on the 3 x 3 ring r of a set pixel (bit d = the neighbour in direction d is set):
 *        links = r & (0x55 | ~(rotl8(r, 1) | rotr8(r, 1))).
 *      deg(p) = popcount(links).  deg <= 4, and the components of the link graph are the 8-connected components.
 *   2. Nodes.  A NODE is a set pixel with deg != 2: an isolated pixel (0), a curve end (1) or a junction (3 or 4).  Every
 *      other set pixel is a PATH PIXEL.
 *   3. Curves.
 *      Isolated pixel p: the curve [p], key 8 * index(p).
 *      Open curve: from a node p along a link in direction d, step to the neighbour; while that pixel is a path pixel,
 *        leave it by its other link.  The walk ends at a node e, entered by a link that points back from e in direction
 *        d' (the last step's direction + 4, mod 8).  p and e may be the same junction: a loop hanging on it.  The path has
 *        two descriptors with the keys 8 * index(p) + d and 8 * index(e) + d', which always differ; the curve is emitted
 *        once, from the smaller key, as p, the path pixels in walking order, e.  So a junction pixel ends deg curves, and
 *        a curve between two adjacent nodes has two points.
 *      Closed curve: a component of the link graph made of path pixels only.  It starts at its smallest index p0, whose
 *        two links lie among directions 0 .. 3, leaves by the smaller of the two, d, and lists every pixel once; p0 is not
 *        repeated.  Its key is 8 * index(p0) + d.
 *      Every link lies on exactly one curve; every path pixel and every isolated pixel is listed exactly once; a node of
 *      degree k >= 1 is listed k times, always as a first or last point; consecutive points are linked.
 *   4. Selection and order.  A curve is kept if it has at least min_length points; min_length <= 1 keeps all.  Dropping a
 *      short curve (a spur) does NOT re-link what remains across the junction: the junction stays a node and the curves
 *      that meet there stay split.  Within a frame the kept curves are ordered by key (start index, then first
 *      direction), ascending; across the batch by frame.
 *   5. Record: CANNY_HIP_CURVE_RECORD = 4 ints per kept curve -- start, end, points, flags (enum canny_hip_curve_field).
 *      For a closed curve `end` is the last listed pixel; for an isolated pixel end == start.  flags: enum
 *      canny_hip_curve_flag; the last direction is that of the step that reaches `end`; both direction fields are 0 when
 *      there is no step.
 *   Outputs, the two-level CSR of the contour chains (all offsets unsigned long long), so that canny_hip_dev_edgels_at,
 *   canny_hip_dev_polygons_chains and canny_hip_dev_shapes_chains take them as they are (the latter two treat every chain
 *   as closed):
 *     offsets[0 .. n_frames]: records per frame, point_offsets[0 .. n_frames]: points per frame -- always the TRUE counts,
 *       both mandatory.  K = offsets[n_frames].  A counts-only call (capacity = 0, point_capacity = 0, the other pointers
 *       NULL) sizes the buffers.
 *     chain_offsets[j] for j = 0 .. min(K, capacity): the points of records 0 .. j - 1, true prefix sums over the whole
 *       batch.  Entries past min(K, capacity) are not written.
 *     points (int): position q is written iff q < point_capacity and it belongs to a record < capacity: a chain may be
 *       cut, nothing is written at or past points + point_capacity.
 *     records (optional, may be NULL at any capacity): 4 ints per curve, bounded by capacity.
 *   points == NULL with point_capacity > 0 and chain_offsets == NULL with capacity > 0 are CANNY_HIP_ERR_INVALID.
 *   The result follows the MAP: max_val > 255 empties every map, so all offsets and point_offsets are 0 (and
 *     chain_offsets[0] = 0 if given).
 *   Limits: height * width <= 2^28, beyond that CANNY_HIP_ERR_UNSUPPORTED before anything is queued (a frame has at most 4
 *     points per pixel and 2 records per pixel, which fit the 32-bit row sums below that).  Otherwise the statuses are
 *     those of canny_hip_dev_canny for the same arguments, which runs first; on a status other than OK nothing is written.
 *   The output is the same bytes on every run and machine: record numbers and positions are prefix sums in key order,
 *     every word is stored once by the one thread that owns its curve, no atomic and no counter hands out space, and the
 *     launches depend on the shapes and on which outputs were asked for, never on the data.
 * Memory: two context workspaces of 4 bytes per image row and 8 bytes per frame (those of the contour chains' scans).
 * Cost: a curve is walked by ONE thread, from both of its ends, in the count pass and again in the write pass, which
 *   walks the owned curves once more to store them; a call takes as long as its longest curve.  DESIGN.md section 28 has
 *   the measured time per step.
 * The two parts are timed by canny_hip_curves_profile_get (CANNY_HIP_CURVE_PART_*); with "profile_stage_mask" they go by
 *   bit 30, like every part added after the polygons.
 * Not covered -- follow-ups: spur pruning WITH re-linking across the junction, an open-curve mode for the polygons and the
 * shape measures, parallel ranking of long curves, the three-stream batch pipeline, the multi-GPU sharder, colour and
 * per-frame / automatic-threshold variants. */
#define CANNY_HIP_CURVE_RECORD 4
enum canny_hip_curve_field {
    CANNY_HIP_CURVE_START = 0,   /* index of the first point */
    CANNY_HIP_CURVE_END = 1,     /* index of the last listed point */
    CANNY_HIP_CURVE_POINTS = 2,  /* number of points */
    CANNY_HIP_CURVE_FLAGS = 3
};
enum canny_hip_curve_flag {
    CANNY_HIP_CURVE_CLOSED = 1,          /* bit 0: a closed curve */
    CANNY_HIP_CURVE_START_JUNCTION = 2,  /* bit 1: the start is a junction (deg >= 3) */
    CANNY_HIP_CURVE_END_JUNCTION = 4,    /* bit 2: the end is a junction */
    CANNY_HIP_CURVE_ISOLATED = 8,        /* bit 3: an isolated pixel */
    CANNY_HIP_CURVE_FIRST_DIR_SHIFT = 4, /* bits 4 .. 6: the direction of the first step */
    CANNY_HIP_CURVE_LAST_DIR_SHIFT = 8,  /* bits 8 .. 10: the direction of the last step */
    CANNY_HIP_CURVE_DIR_MASK = 7
};
enum canny_hip_curve_part {
    CANNY_HIP_CURVE_PART_COUNT = 0,  /* first walks: kept curves and their points per row, scanned: offsets, point_offsets */
    CANNY_HIP_CURVE_PART_WRITE = 1,  /* the walks again: record numbers and chain_offsets, then records and points stored */
    CANNY_HIP_CURVE_PARTS = 2
};
/* Device buffers, asynchronous; completion contract and d_edges as canny_hip_dev_canny_points.  canny_hip_dev_canny itself
 * queues exactly what it queues on its own; the walks read the converged hysteresis bit-plane behind it. */
int canny_hip_dev_canny_curves(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                               int height, int width, int n_frames, short *d_edges, int min_length, int *d_records,
                               unsigned long long capacity, unsigned long long *d_offsets,
                               unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                               unsigned long long *d_point_offsets);
/* The curves alone, on device bit maps in the layout of canny_hip_dev_canny_bits (rows MSB-first, padded to bytes; any
 * byte alignment; the padding bits of a row are ignored, whatever they hold).  Asynchronous. */
int canny_hip_dev_curves_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                              int min_length, int *d_records, unsigned long long capacity, unsigned long long *d_offsets,
                              unsigned long long *d_chain_offsets, int *d_points, unsigned long long point_capacity,
                              unsigned long long *d_point_offsets);
/* Host buffers, synchronous: upload, canny, curves; offsets and point_offsets come down first, then what fits:
 * min(K, capacity) + 1 chain offsets, as many records, and the points below min(chain_offsets[min(K, capacity)],
 * point_capacity). */
int canny_hip_canny_curves(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int min_length, int *records, unsigned long long capacity,
                           unsigned long long *offsets, unsigned long long *chain_offsets, int *points,
                           unsigned long long point_capacity, unsigned long long *point_offsets);
/* Host-only, needs no device: the same rule on ONE host bit map, in plain C++.  *count receives the true number of kept
 * curves, *point_count the true number of their points; both are mandatory. */
int canny_hip_curves_from_bits(const unsigned char *bits, int height, int width, int min_length, int *records,
                               unsigned long long capacity, unsigned long long *count, unsigned long long *chain_offsets,
                               int *points, unsigned long long point_capacity, unsigned long long *point_count);

/* ---- Euclidean distance transform ----------------------------------------------------------------------------------------
 * For every pixel of every frame the distance to the nearest edge pixel, on the GPU, queued behind the detector on the same
 * stream with no host round trip: what chamfer and template matching, edge-based registration, "snap to the nearest edge" and
 * contour-deviation scores start from.  THE RULE, for frame f with edge map E_f (the map
 * canny_hip_canny returns for that frame, bit for bit) and S_f = { (r', c') : E_f[r'][c'] != 0 }:
 *   dist2 (int, [n][height][width]): dist2[r][c] = min over (r', c') in S_f of (r - r')^2 + (c - c')^2 -- an integer, so the
 *     transform is EXACT; 0 on edge pixels.
 *   nearest (int, same shape): the index r' * width + c' of a pixel of S_f that attains that minimum; where several do, the
 *     smallest index.  On an edge pixel its own index.
 *   dist (float, same shape): (float)sqrt((double)dist2), the correctly rounded single-precision root, computed in double on
 *     the device (dist2 exceeds 2^24 on large frames: a float root of a float-converted dist2 is NOT the rule).  It equals
 *     numpy.sqrt(dist2.astype(float64)).astype(float32) and scipy.ndimage.distance_transform_edt(~mask).astype(float32)
 *     bit for bit, and is what cv::distanceTransform(DIST_L2, DIST_MASK_PRECISE) approximates.
 *   A frame without edge pixels: every dist2 is CANNY_HIP_EDT_NONE, every dist +inf, every nearest -1.  The result follows
 *     the MAP, not the plane it is derived from: max_val > 255 empties every map (see the point lists).
 *   Any of the three output pointers may be NULL, and what the others receive does not depend on that; all three NULL is
 *     CANNY_HIP_ERR_INVALID.  Every element of every plane given is written, nothing beyond it.
 *   Limits: height * width < 2^31 and height^2 + width^2 < 2^31 (dist2 and the indices are 32-bit); beyond that
 *     CANNY_HIP_ERR_UNSUPPORTED, before anything is queued.  Otherwise the statuses of the canny forms are those of
 *     canny_hip_dev_canny for the same arguments, which runs first; on a status other than OK nothing is written.
 *   The output is the same bytes on every run: there are no atomics, every element is stored once by one thread, and the
 *     launches depend on the shapes and on which planes were asked for, never on the data.  The work per frame is
 *     O(height * width) whatever the map holds (one edge pixel or none included).
 * Memory: a context workspace of 2 bytes per pixel (rows padded to 64 pixels) holds the row pass's result; with
 *   dist2 == NULL another 4 bytes per pixel hold the column scan's stack, which otherwise lives in the dist2 plane itself.
 * The two parts are timed by canny_hip_edt_profile_get (CANNY_HIP_EDT_PART_*); with "profile_stage_mask" they are bits 17
 *   and 18.
 * Not covered -- follow-ups: truncated or u8 outputs, L1 / chessboard metrics, the distance to the nearest NON-edge pixel,
 * the three-stream batch pipeline, the multi-GPU sharder, colour and per-frame / automatic-threshold variants. */
#define CANNY_HIP_EDT_NONE 0x7FFFFFFF
enum canny_hip_edt_part {
    CANNY_HIP_EDT_PART_ROWS = 0,     /* per row: the column of the nearest set pixel of that row (u16 workspace) */
    CANNY_HIP_EDT_PART_COLUMNS = 1,  /* per column: lower envelope of the rows' parabolas; the planes are stored */
    CANNY_HIP_EDT_PARTS = 2
};
/* Device buffers, asynchronous; completion contract and d_edges as canny_hip_dev_canny_points.  canny_hip_dev_canny itself
 * queues exactly what it queues on its own; the transform reads the converged hysteresis bit-plane behind it, never the
 * s16 map. */
int canny_hip_dev_canny_edt(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                            int height, int width, int n_frames, short *d_edges, int *d_dist2, float *d_dist,
                            int *d_nearest);
/* The transform alone, on device bit maps in the layout of canny_hip_dev_canny_bits (rows MSB-first, padded to bytes; any
 * byte alignment; the padding bits of a row are ignored, whatever they hold).  Asynchronous. */
int canny_hip_dev_edt_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int height, int width, int n_frames,
                           int *d_dist2, float *d_dist, int *d_nearest);
/* Host buffers, synchronous: upload, canny, transform; only the planes that were asked for come down. */
int canny_hip_canny_edt(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                        int height, int width, int *dist2, float *dist, int *nearest);
/* Host-only, needs no device: the same rule on ONE host bit map, in plain C++ (the same two passes) -- what a caller of
 * canny_hip_canny_batch_bits runs on the maps it received. */
int canny_hip_edt_from_bits(const unsigned char *bits, int height, int width, int *dist2, float *dist, int *nearest);

/* ---- chamfer template matching -------------------------------------------------------------------------------------------
 * Where does a given shape sit in a frame?  Given a set of point templates, every finished edge map gets, per frame, the
 * truncated chamfer score of every template at every anchor, its local minima under a mean-cost threshold, and an ordered,
 * distance-suppressed list of matches -- on the GPU behind the distance transform, on the same stream, with no host round
 * trip.  All integers: the same bytes on every run and every machine.  tests/chamfer_rule.py restates the rule in numpy,
 * csrc/canny_chamfer_host.cpp in plain C++.  THE RULE:
 *   Templates: a set of T templates, 1 <= T <= CANNY_HIP_CHAMFER_MAX_TEMPLATES, CSR-shaped: offsets holds T + 1 ints,
 *     offsets[0] = 0, non-decreasing; points holds offsets[T] pairs of shorts (dx, dy) = (column offset, row offset) from the
 *     template's anchor.  Template t has K_t = offsets[t + 1] - offsets[t] points, 1 <= K_t <= 65536; offsets[T] <= 2^20;
 *     |dx|, |dy| <= CANNY_HIP_CHAMFER_MAX_EXTENT.  Duplicates are allowed and count as often as they occur.  (The sum below is
 *     an integer sum: the set stores the points in the order its kernels like.)
 *   Cost: cost(d2) = min(isqrt(d2 * 256), trunc_q4): isqrt is the floor integer square root of the 64-bit product, i.e. the
 *     distance in 1/16 pixel, truncated; 1 <= trunc_q4 <= 4095.  d2 = CANNY_HIP_EDT_NONE gives trunc_q4 (isqrt(2^39) > 4095),
 *     so a frame with an empty map -- max_val > 255 included: the result follows the MAP -- costs trunc_q4 everywhere.
 *   Score, for frame f, template t and anchor (y, x) anywhere in the frame:
 *     S[f][t][y][x] = sum over the template's points k of cost_f(y + dy_k, x + dx_k),
 *     where a point that falls outside the frame contributes trunc_q4.  S <= 4095 * 65536 < 2^28.
 *   Candidates: (t, y, x) is a candidate iff
 *     1. S <= max_mean_q4 * K_t, the mean-cost threshold in 1/16 pixel, 0 <= max_mean_q4 < trunc_q4 (the strict bound keeps
 *        saturated plateaus out), and
 *     2. S is a five-way local minimum in its own template's plane, mirroring the Hough peak rule:
 *        S < left && S <= right && S < up && S <= down, neighbours outside the frame counting as +infinity (on a plateau
 *        the first pixel in raster order wins).
 *   Order: mean_q12 = floor(S * 256 / K_t) (64 bits); base = t * height * width + y * width + x, with
 *     T * height * width < 2^31 (beyond: CANNY_HIP_ERR_UNSUPPORTED).  The candidates are sorted by (mean_q12 ascending, base
 *     ascending); the first min(matches_max, n_candidates) go on, 1 <= matches_max <= CANNY_HIP_HOUGH_MAX_LINES.
 *   Acceptance (the pattern of the circles): the candidates are taken in that order; one is accepted iff no earlier ACCEPTED
 *     one, of whatever template, has (dx)^2 + (dy)^2 < min_dist^2.  min_dist >= 0; 0 disables the check.
 *   Output: frame f writes its accepted matches compactly, in that order, to slots f * matches_max + j of matches; a match is
 *     CANNY_HIP_MATCH_INTS = 6 ints: x, y, template, score, mean_q12, base.  counts[f] (mandatory) is the number accepted,
 *     cand_counts[f] (may be NULL) the true number of candidates; later slots are not written.  matches may be NULL (counts
 *     only).  d_scores, if given, is [n][T][height][width] unsigned ints and receives every S; what the other outputs hold
 *     does not depend on whether it is given.
 *   Statuses: bad ranges (trunc_q4 < 1, max_mean_q4 outside 0 .. trunc_q4 - 1, min_dist < 0, matches_max < 1, sizes < 1),
 *     NULL mandatory pointers, a bad template set (offsets[0] != 0, a template without points, no template; for the device
 *     forms a set of another context or a destroyed one): CANNY_HIP_ERR_INVALID; over a documented limit (trunc_q4 > 4095,
 *     matches_max > CANNY_HIP_HOUGH_MAX_LINES, more than 1024 templates, 65536 points in one or 2^20 in all, a point of
 *     extent 256, T * height * width >= 2^31, and for the device forms height or width > 65535):
 *     CANNY_HIP_ERR_UNSUPPORTED; both before anything is queued, nothing is written.  Otherwise the detector's or the
 *     transform's own status comes first.  A dist2 word is read as unsigned: a negative one costs trunc_q4.
 *   The context option "chamfer_route" chooses the score kernel: 0 automatic, 1 direct (one lane per anchor, costs gathered
 *     from the cost plane in memory), 2 tiled (the cost tile with the template's halo in LDS).  Same bytes either way.
 * Memory: the batch is walked in CHUNKS of whole frames, a function of the shapes alone: at most 4096 frames, and no more
 *   than keep the larger per-chunk workspace within 256 MiB (one frame at least, whatever it takes).  That workspace is
 *   the scores, 4 B per template and pixel, or, with d_scores given, the u16 cost plane, 2 B per pixel (which is there in
 *   both cases).  A third workspace holds, per frame of the chunk, the cut-off's histogram and the collected keys:
 *   32 KiB + 8 * matches_max bytes, 256 MiB at 4096 frames and 4096 matches.  With d_dist2 == NULL the canny and bits forms
 *   keep the dist2 plane of the WHOLE batch in a fourth, 4 B per pixel.
 * The four parts are timed by canny_hip_chamfer_profile_get (CANNY_HIP_CHAMFER_PART_*); with "profile_stage_mask" they go
 *   by bit 30 like every part behind the polygons.
 * Not covered -- follow-ups: oriented chamfer (the edgels' directions), anchor strides and coarse-to-fine search, sub-pixel
 * match refinement, the three-stream batch pipeline, the multi-GPU sharder, colour and per-frame-threshold variants. */
#define CANNY_HIP_CHAMFER_MAX_EXTENT 255
#define CANNY_HIP_CHAMFER_MAX_TEMPLATES 1024
#define CANNY_HIP_CHAMFER_MAX_POINTS 65536      /* per template */
#define CANNY_HIP_CHAMFER_MAX_TOTAL (1 << 20)   /* points of a set */
#define CANNY_HIP_CHAMFER_MAX_TRUNC 4095
#define CANNY_HIP_MATCH_INTS 6
enum canny_hip_chamfer_part {
    CANNY_HIP_CHAMFER_PART_COST = 0,        /* dist2 -> u16 cost plane */
    CANNY_HIP_CHAMFER_PART_SCORE = 1,       /* the sliding sums */
    CANNY_HIP_CHAMFER_PART_CANDIDATES = 2,  /* local minima, cut-off (radix select on the keys), collect */
    CANNY_HIP_CHAMFER_PART_ACCEPT = 3,      /* sort + ordered acceptance, one workgroup per frame */
    CANNY_HIP_CHAMFER_PARTS = 4
};
typedef struct canny_hip_chamfer_set canny_hip_chamfer_set;
/* Validates, uploads once and precomputes what the launches need (K_t, bounding boxes, the points sorted by (dy, dx) and
 * cut into bands of dy whose halo fits in LDS).  A set belongs to its context and dies with it at the latest; destroy
 * synchronises the context's stream first.  Synchronous. */
int canny_hip_chamfer_set_create(canny_hip_ctx *ctx, const int *offsets, const short *points, int n_templates,
                                 canny_hip_chamfer_set **set);
int canny_hip_chamfer_set_destroy(canny_hip_ctx *ctx, canny_hip_chamfer_set *set);
/* Matching alone on a device dist2 plane ([n][height][width] ints, what canny_hip_dev_canny_edt writes).  Any height,
 * width >= 1.  Asynchronous. */
int canny_hip_dev_chamfer_dist2(canny_hip_ctx *ctx, const int *d_dist2, int n_frames, int height, int width,
                                const canny_hip_chamfer_set *set, int trunc_q4, int max_mean_q4, int min_dist,
                                int matches_max, int *d_matches, int *d_counts, int *d_cand_counts, unsigned int *d_scores);
/* canny_hip_dev_edt_bits unchanged, then the matching.  d_dist2 may be the caller's plane or NULL (a workspace then). */
int canny_hip_dev_chamfer_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int height, int width,
                               int *d_dist2, const canny_hip_chamfer_set *set, int trunc_q4, int max_mean_q4, int min_dist,
                               int matches_max, int *d_matches, int *d_counts, int *d_cand_counts, unsigned int *d_scores);
/* canny_hip_dev_canny_edt unchanged (d_edges, d_dist2 as there; either may be NULL), then the matching, on the same
 * stream. */
int canny_hip_dev_canny_chamfer(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                int height, int width, int n_frames, short *d_edges, int *d_dist2,
                                const canny_hip_chamfer_set *set, int trunc_q4, int max_mean_q4, int min_dist,
                                int matches_max, int *d_matches, int *d_counts, int *d_cand_counts, unsigned int *d_scores);
/* Host buffers, synchronous, in the pattern of canny_hip_canny_hough_circles: the counts come down first, then only the
 * filled slots of matches.  matches and cand_counts may be NULL. */
int canny_hip_canny_chamfer(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                            int max_val, int height, int width, const canny_hip_chamfer_set *set, int trunc_q4,
                            int max_mean_q4, int min_dist, int matches_max, int *matches, int *counts, int *cand_counts);
/* Host-only, needs no device: the rule on ONE host dist2 plane with host template arrays, in plain C++.  matches
 * (matches_max * 6 ints; only the accepted records are written) and cand_count may be NULL; scores, if given, receives
 * n_templates * height * width unsigned ints. */
int canny_hip_chamfer_from_dist2(const int *dist2, int height, int width, const int *offsets, const short *points,
                                 int n_templates, int trunc_q4, int max_mean_q4, int min_dist, int matches_max,
                                 int *matches, int *count, int *cand_count, unsigned int *scores);
/* Host-only: cost(d2) of the rule; -1 for d2 < 0 or trunc_q4 outside 1..4095. */
int canny_hip_chamfer_cost_of(int d2, int trunc_q4);
/* Test hook: the device's cost arithmetic alone on n dist2 values; d_costs receives n unsigned ints.  trunc_q4 in
 * 1..4095 runs the cost pass's own function; trunc_q4 = 0 stores the untruncated root isqrt(d2 * 256), which the device
 * takes in floating point and corrects to the exact integer root.  Asynchronous. */
int canny_hip_dev_chamfer_costs(canny_hip_ctx *ctx, const int *d_dist2, size_t n, int trunc_q4, unsigned int *d_costs);

/* ---- corners (Harris / Shi-Tomasi) ----------------------------------------------------------------------------------------
 * Where are the corners of a frame?  What cv::goodFeaturesToTrack and cv::cornerHarris answer, computed per frame from the
 * smoothed plane every canny call leaves on the device: a structure-tensor response at every pixel, its local maxima over
 * a quality threshold, and an ordered, distance-suppressed list of corners -- on the GPU, on the same stream, with no host
 * round trip.  All integers: the same bytes on every run and every machine.  tests/corners_rule.py restates the rule in
 * numpy and in plain Python ints, csrc/canny_corners_host.cpp in plain C++.  THE RULE:
 *   Plane: P is a u8 plane of height x width, height, width >= 2.  (The context's own plane may be s16 when option
 *     "smoothed_u8" is 0; the Gaussian keeps its values in [0, 255], and the bounds below rest on that: a caller's plane is
 *     u8 only.)
 *   Gradient: (gx, gy) = the reference's 3 x 3 Sobel pair at (y, x) with its border rules (gx clamps columns and drops
 *     rows outside the frame, gy clamps rows and drops columns), as for the edgels and the circles.  |gx|, |gy| <= 1020.
 *   Tensor, for block in {3, 5, 7}, r = block / 2: Sxx(y, x) = the sum of gx^2 over the block x block window centred on
 *     (y, x), Syy that of gy^2, Sxy that of gx * gy; a window position outside the frame contributes 0.
 *     Sxx, Syy <= 49 * 1020^2 = 50,979,600 = CANNY_HIP_CORNERS_MAX_SUM and |Sxy| <= the same: all three fit in an int.
 *   Response R, a signed 64-bit value:
 *     CANNY_HIP_CORNERS_MIN_EIGEN (Shi-Tomasi): R = Sxx + Syy - ceil_sqrt(D), D = (Sxx - Syy)^2 + 4 * Sxy^2 < 2^54,
 *       ceil_sqrt the exact integer ceiling root: R = floor(2 * lambda_min), 0 <= R < 2^27.  k_q8 must be 0.
 *     CANNY_HIP_CORNERS_HARRIS: R = 256 * (Sxx * Syy - Sxy^2) - k_q8 * (Sxx + Syy)^2, 0 <= k_q8 <= 64 (10 is k ~ 0.04);
 *       both terms stay below 6.7e17, |R| < 2^61, and a positive R is below 2^60.
 *   Threshold: Rmax[f] = the largest R of frame f over all its pixels; thr[f] = floor(max(Rmax, 0) * quality_q16 / 65536),
 *     0 <= quality_q16 <= 65536 (the product is taken exactly, beyond 64 bits); min_response >= 0 is an absolute floor.
 *   Candidates: (y, x) is a candidate iff R >= max(thr, min_response, 1), and R > each of the four 3 x 3 neighbours that
 *     precede it in raster order (up-left, up, up-right, left), and R >= each of the four that follow it; neighbours
 *     outside the frame are ignored.  On a plateau the first pixel in raster order wins (the Hough peak rule taken to
 *     eight neighbours).
 *   Order: base = y * width + x; the candidates are sorted by (R descending, base ascending); the first
 *     min(corners_max, n_candidates) go on, 1 <= corners_max <= CANNY_HIP_HOUGH_MAX_LINES.
 *   Acceptance (the pattern of the chamfer matches and the circles): the selected candidates are taken in that order; one
 *     is accepted iff no earlier ACCEPTED one has dx^2 + dy^2 < min_dist^2.  min_dist >= 0; 0 disables the check.
 *   Output: frame f writes its accepted corners compactly, in that order, to slots f * corners_max + j of corners; a
 *     corner is CANNY_HIP_CORNER_WORDS = 4 long long: x, y, response, rank -- rank its position in the selected order, so a
 *     caller sees what the distance rule removed.  counts[f] (mandatory) is the number accepted, cand_counts[f] (may be
 *     NULL) the true number of candidates, max_response[f] (may be NULL) Rmax; later slots are not written.  d_response, if
 *     given, is [n][height][width] long long and receives every R; what the other outputs hold does not depend on whether
 *     it is given.
 *   Statuses: bad ranges (block, mode, k_q8, quality_q16, min_response, min_dist, corners_max < 1, sizes < 1), NULL
 *     mandatory pointers (the corner records are mandatory), frames under 2 x 2, a record or response buffer that is not
 *     8-byte aligned: CANNY_HIP_ERR_INVALID; over a documented limit (corners_max > CANNY_HIP_HOUGH_MAX_LINES,
 *     height * width >= 2^31, and for the device forms height or width > 65535): CANNY_HIP_ERR_UNSUPPORTED; both before
 *     anything is queued, nothing is written.  Otherwise the detector's own status comes first.  max_val > 255 empties
 *     the MAP but not the corners: the result follows the PLANE.
 * Memory: the response plane is not kept (16 B/px stored and read back against 1 B/px per pass over the plane): the
 *   response is computed again wherever it is needed.  The batch is walked in chunks of at most 1024 frames; the workspace
 *   holds, per frame of a chunk, a histogram of 32 KiB, the collected keys (16 * corners_max bytes), a list of the frame's
 *   candidate keys (16 bytes each, min(16384, ceil(height / 2) * ceil(width / 2)) of them: a frame with more candidates
 *   than corners_max AND than the list holds computes its responses once more per 13 bits of the key) and a few words.
 * The four parts are timed by canny_hip_corners_profile_get (CANNY_HIP_CORNER_PART_*); with "profile_stage_mask" they go
 *   by bit 30 like every part behind the polygons.
 * Not covered -- follow-ups: sub-pixel corner refinement (cornerSubPix); a mask, such as corners only near edge pixels of
 * the finished map; block sizes above 7; Gaussian-weighted windows; s16 caller planes; colour, per-frame and
 * automatic-threshold forms; the three-stream batch pipeline; the multi-GPU sharder. */
#define CANNY_HIP_CORNER_WORDS 4
#define CANNY_HIP_CORNERS_MAX_SUM 50979600
#define CANNY_HIP_CORNERS_MAX_K_Q8 64
enum canny_hip_corners_mode { CANNY_HIP_CORNERS_MIN_EIGEN = 0, CANNY_HIP_CORNERS_HARRIS = 1 };
enum canny_hip_corner_part {
    CANNY_HIP_CORNER_PART_MAX = 0,         /* pass 1: every R, the frame's maximum, the response plane if asked for */
    CANNY_HIP_CORNER_PART_CANDIDATES = 1,  /* pass 2: R again, threshold, local maxima; the cut-off's digit histograms */
    CANNY_HIP_CORNER_PART_COLLECT = 2,     /* pass 2 once more: every key up to the cut-off */
    CANNY_HIP_CORNER_PART_ACCEPT = 3,      /* sort + ordered acceptance, one workgroup per frame */
    CANNY_HIP_CORNER_PARTS = 4
};
/* canny_hip_dev_canny unchanged (d_edges as there), then the corners of the smoothed plane it left, on the same stream.
 * d_corners: n_frames * corners_max * 4 long long.  Asynchronous. */
int canny_hip_dev_canny_corners(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val, int max_val,
                                int height, int width, int n_frames, short *d_edges, int mode, int block, int k_q8,
                                int quality_q16, long long min_response, int min_dist, int corners_max,
                                long long *d_corners, int *d_counts, int *d_cand_counts, long long *d_max_response,
                                long long *d_response);
/* The corners of a caller's device u8 plane ([n][height][width] bytes).  With d_plane == NULL: of the plane the context's
 * last canny call left, under the rule of canny_hip_dev_edgels_at -- a context that ran no such call, or a call for
 * another shape, gives CANNY_HIP_ERR_INVALID with nothing queued.  Asynchronous. */
int canny_hip_dev_corners_plane(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int height, int width,
                                int mode, int block, int k_q8, int quality_q16, long long min_response, int min_dist,
                                int corners_max, long long *d_corners, int *d_counts, int *d_cand_counts,
                                long long *d_max_response, long long *d_response);
/* Host buffers, synchronous, in the pattern of canny_hip_canny_chamfer: the counts come down first, then only the filled
 * slots of corners.  cand_counts and max_response may be NULL. */
int canny_hip_canny_corners(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                            int max_val, int height, int width, int mode, int block, int k_q8, int quality_q16,
                            long long min_response, int min_dist, int corners_max, long long *corners, int *counts,
                            int *cand_counts, long long *max_response);
/* Host-only, needs no device: the rule on ONE host u8 plane, in plain C++.  corners (corners_max * 4 long long; only the
 * accepted records are written) and count are mandatory; cand_count, max_response and response (height * width long
 * long) may be NULL. */
int canny_hip_corners_from_plane(const unsigned char *plane, int height, int width, int mode, int block, int k_q8,
                                 int quality_q16, long long min_response, int min_dist, int corners_max,
                                 long long *corners, int *count, int *cand_count, long long *max_response,
                                 long long *response);
/* Host-only: R of the rule for one tensor (0 <= sxx, syy <= CANNY_HIP_CORNERS_MAX_SUM, |sxy| <= the same; otherwise, or
 * with a bad mode or k_q8, CANNY_HIP_ERR_INVALID and *r untouched). */
int canny_hip_corner_response_of(int sxx, int syy, int sxy, int mode, int k_q8, long long *r);
/* Test hook: the device's response function alone on n triples (d_sums: n * 3 ints sxx, syy, sxy within the bounds above;
 * d_r receives n long long).  Asynchronous. */
int canny_hip_dev_corners_arith(canny_hip_ctx *ctx, const int *d_sums, size_t n, int mode, int k_q8, long long *d_r);

/* ---- corner descriptors and Hamming matching --------------------------------------------------------------------------------
 * Which corner of this frame is which corner of the next?  A binary descriptor per corner -- 256 intensity comparisons on the
 * smoothed plane, optionally steered by the patch's intensity centroid: the BRIEF / ORB idea, with a pattern and rounding of
 * the library's own -- and a brute-force Hamming matcher between the descriptor sets of pairs of frames (best and
 * second-best neighbour, distance, ratio and mutual tests: what cv::BFMatcher(NORM_HAMMING) with knnMatch(k = 2) and
 * crossCheck answer).  On the GPU, on the context's stream, no host round trip, no atomics.  All integers: the same bytes on
 * every run and every machine.  tests/descriptors_rule.py restates the rule in numpy and plain Python ints,
 * csrc/canny_descriptors_host.cpp in plain C++.  THE RULE:
 *   Plane: P is a u8 plane of height x width, height, width >= 2.  (The context's own plane may be s16 with values in
 *     [0, 255], as for the corners; a caller's plane is u8 only.)  Every read is
 *     P(clamp(y + dy, 0, height - 1), clamp(x + dx, 0, width - 1)): every corner gets a descriptor, nothing is read
 *     outside the plane.
 *   Corners: the 4-word records (x, y, response, rank) of the corners calls at slots f * corners_max + j, j < counts[f];
 *     only x and y are read.  A record whose x or y lies outside the frame reads nothing: its descriptor is four zero words
 *     and its meta word is -1.
 *   Pattern (CANNY_HIP_DESC_BITS = 256 tests, CANNY_HIP_DESC_RADIUS = 15): a generator with state s = 0x43414E59.  A draw
 *     is s = (s * 1664525 + 1013904223) mod 2^32, then v = (s >> 16) % 27 - 13.  An attempt draws ax, ay, bx, by in that
 *     order and is rejected if ax^2 + ay^2 > 169 or bx^2 + by^2 > 169, or |ax - bx| + |ay - by| < 4, or the pair was
 *     already taken, in either order; 256 tests exist after 491 attempts.
 *   Rotation k of CANNY_HIP_DESC_ROTATIONS = 32: rot_k(x, y) = (rd(x * C_k - y * S_k), rd(x * S_k + y * C_k)),
 *     rd(v) = floor((v + 8192) / 16384); C_k = cos(2 pi k / 32) in Q14 from the nine constants 16384, 16069, 15137, 13623,
 *     11585, 9102, 6270, 3196, 0 by symmetry, S_k = C_(k - 8); y points down.  Every rotated offset stays within +-13, the
 *     256 tests stay distinct in every rotation, no test has both ends equal, and rotation k + 8 is exactly the 90-degree
 *     rotation (x, y) -> (-y, x) of rotation k, for every k.  The 32 x 256 x 4 signed bytes are data in
 *     csrc/canny_desc_pattern.h; canny_hip_descriptor_pattern returns one rotation.
 *   Orientation (option CANNY_HIP_DESC_STEERED): m10 = sum of dx * P, m01 = sum of dy * P over the 709 offsets with
 *     dx^2 + dy^2 <= 225 (clamped reads); k = the smallest index that maximises m10 * C_k + m01 * S_k, in 64 bits; a flat
 *     patch gives k = 0.  Without the option k = 0.
 *   Descriptor: bit t % 64 of word t / 64 is 1 iff P(corner + rot_k(a_t)) < P(corner + rot_k(b_t)).  desc is
 *     [n][corners_max][4] unsigned long long, meta [n][corners_max] int = k + 256 * border, border = 1 iff the 31 x 31 patch
 *     leaves the frame.  Slots past counts[f] are not written.
 *   Matching: a query set and a train set, each descriptor words ([frames][stride][4]), per-frame counts and a slot stride,
 *     0 <= counts <= stride (a count outside is clamped into that range), 1 <= stride <= CANNY_HIP_HOUGH_MAX_LINES; the two
 *     sets may be the same buffers.  n_pairs pairs (q frame, t frame), 2 ints each, as a HOST array: the call copies it,
 *     so the frame indices are validated before anything is queued.  For query i of a pair: d(i, j) = the popcount of the
 *     XOR of the four words; the best neighbour is the j with the smallest (d, j), d1 its distance; d2 the smallest
 *     distance among j != best (it may equal d1; 257 if there is none); an empty train set gives j = -1, d1 = d2 = 257.
 *   Flags: bit 0: d1 <= max_distance (0..256).  bit 1: ratio_q8 == 0 or d1 * 256 < ratio_q8 * d2 (ratio_q8 0..256; 205 is
 *     Lowe's 0.8).  bit 2, mutual: i is the query with the smallest (d(i', j), i') for its best j; always computed.
 *     bit 3, accepted: bits 0 and 1, and bit 2 if option CANNY_HIP_MATCH_CROSS_CHECK is set.
 *   Output: matches is [n_pairs][stride_q][CANNY_HIP_MATCH_WORDS = 4] int: j, d1, d2, flags; slots past the query count are
 *     not written.  pair_counts[p] = the number accepted.
 *   Statuses: bad ranges, NULL mandatory pointers, descriptor or record buffers that are not 8-byte aligned, pair indices
 *     outside the sets: CANNY_HIP_ERR_INVALID; over a documented limit (corners_max or a stride >
 *     CANNY_HIP_HOUGH_MAX_LINES, height * width >= 2^31, more than 65535 frames, more than 2^20 pairs):
 *     CANNY_HIP_ERR_UNSUPPORTED; both before anything is queued, nothing is written.
 * Memory: the matcher's workspace holds the pairs and one int per (pair, train slot).
 * The four parts are timed by canny_hip_descriptors_profile_get (CANNY_HIP_DESC_PART_*); with "profile_stage_mask" they go
 *   by bit 30 like every part behind the polygons.
 * Geometric verification (RANSAC) of the matches: canny_hip_dev_estimate_motion below.
 * Not covered -- follow-ups: scale pyramids; sub-pixel corner refinement; matching through the batch pipeline or the
 * multi-GPU sharder. */
#define CANNY_HIP_DESC_BITS 256
#define CANNY_HIP_DESC_WORDS 4
#define CANNY_HIP_DESC_RADIUS 15
#define CANNY_HIP_DESC_ROTATIONS 32
#define CANNY_HIP_MATCH_WORDS 4
#define CANNY_HIP_MATCH_MAX_PAIRS 1048576
enum canny_hip_desc_option { CANNY_HIP_DESC_STEERED = 1 };
enum canny_hip_match_option { CANNY_HIP_MATCH_CROSS_CHECK = 1 };
enum canny_hip_desc_part {
    CANNY_HIP_DESC_PART_DESCRIBE = 0, /* patch, orientation, 256 tests: one wave per corner */
    CANNY_HIP_DESC_PART_MATCH = 1,    /* best and second-best train descriptor of every query */
    CANNY_HIP_DESC_PART_REVERSE = 2,  /* best query of every train descriptor */
    CANNY_HIP_DESC_PART_FINALIZE = 3, /* flags and accepted counts */
    CANNY_HIP_DESC_PARTS = 4
};
/* canny_hip_dev_canny_corners unchanged (d_edges and the corner outputs exactly as there), then the descriptors of the
 * corners on the smoothed plane, on the same stream.  d_desc: n_frames * corners_max * 4 unsigned long long; d_meta:
 * n_frames * corners_max int; both mandatory.  Asynchronous. */
int canny_hip_dev_canny_corner_descriptors(canny_hip_ctx *ctx, const unsigned char *d_img, float sigma, int min_val,
                                           int max_val, int height, int width, int n_frames, short *d_edges, int mode,
                                           int block, int k_q8, int quality_q16, long long min_response, int min_dist,
                                           int corners_max, long long *d_corners, int *d_counts, int *d_cand_counts,
                                           long long *d_max_response, long long *d_response, int desc_options,
                                           unsigned long long *d_desc, int *d_meta);
/* The descriptors of device records and counts on a caller's device u8 plane ([n][height][width] bytes).  With
 * d_plane == NULL: on the plane the context's last canny call left, under the rule of canny_hip_dev_edgels_at -- a context
 * that ran no such call, or a call for another shape, gives CANNY_HIP_ERR_INVALID with nothing queued.  Asynchronous. */
int canny_hip_dev_corner_descriptors(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int height, int width,
                                     const long long *d_corners, const int *d_counts, int corners_max, int desc_options,
                                     unsigned long long *d_desc, int *d_meta);
/* Host buffers, synchronous: the counts come down first, then only the filled slots of corners, desc and meta. */
int canny_hip_canny_corner_descriptors(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma,
                                       int min_val, int max_val, int height, int width, int mode, int block, int k_q8,
                                       int quality_q16, long long min_response, int min_dist, int corners_max,
                                       int desc_options, long long *corners, int *counts, unsigned long long *desc,
                                       int *meta);
/* Host-only, needs no device: the descriptor rule for `count` records (4 long long each) on ONE host u8 plane, in plain
 * C++.  desc receives count * 4 words, meta count ints.  0 <= count <= CANNY_HIP_HOUGH_MAX_LINES. */
int canny_hip_corner_descriptors_from_plane(const unsigned char *plane, int height, int width, const long long *corners,
                                            int count, int options, unsigned long long *desc, int *meta);
/* Host-only: the 256 x 4 signed bytes (ax, ay, bx, by) of rotation k, 0 <= k < 32. */
int canny_hip_descriptor_pattern(int k, signed char *out);
/* The matcher.  pairs is a HOST array of 2 * n_pairs ints (q frame, t frame), 0 <= q frame < n_q_frames, 0 <= t frame <
 * n_t_frames; every other pointer is a device pointer.  d_matches: n_pairs * stride_q * 4 ints; d_pair_counts: n_pairs
 * ints.  Asynchronous. */
int canny_hip_dev_match_descriptors(canny_hip_ctx *ctx, const unsigned long long *d_q_desc, const int *d_q_counts,
                                    int n_q_frames, int stride_q, const unsigned long long *d_t_desc, const int *d_t_counts,
                                    int n_t_frames, int stride_t, const int *pairs, int n_pairs, int max_distance,
                                    int ratio_q8, int options, int *d_matches, int *d_pair_counts);
/* Host-only, needs no device: the matching rule on ONE pair of host descriptor sets (n_q, n_t descriptors of 4 words).
 * matches receives n_q * 4 ints, *accepted the number accepted. */
int canny_hip_match_descriptors(const unsigned long long *q_desc, int n_q, const unsigned long long *t_desc, int n_t,
                                int max_distance, int ratio_q8, int options, int *matches, int *accepted);

/* ---- frame-to-frame motion from the corner matches (RANSAC) -------------------------------------------------------------------
 * How did the camera move between these two frames?  The accepted matches of a pair of frames are verified by consensus and
 * one motion model is fitted to the ones that agree -- what cv::estimateAffinePartial2D / cv::estimateAffine2D answer -- on
 * the GPU, on the context's stream, no host round trip, no atomics.  All integers: the same bytes on every run and every
 * machine.  tests/motion_rule.py restates the rule in numpy and plain Python ints, csrc/canny_motion_host.cpp in plain C++.
 * THE RULE:
 *   Inputs per pair p = (q frame, t frame): the corner records of both frames ([frames][stride][4] long long; only x and y
 *     are read), the per-frame counts (clamped to [0, stride], as in the matcher), and the matcher's output row
 *     [stride_q][4] int (j, d1, d2, flags).  1 <= stride <= CANNY_HIP_HOUGH_MAX_LINES = 4096.
 *   Correspondences: the query slots i < count_q in ascending i; slot i is a correspondence iff flags & 8 (accepted),
 *     0 <= j < count_t, and all four coordinates lie in [0, 65535].  It is c = (x, y, x', y'); m is their number.
 *   Models: CANNY_HIP_MOTION_TRANSLATION = 0 (sample size k = 1), CANNY_HIP_MOTION_SIMILARITY = 1 (k = 2: rotation, uniform
 *     scale, shift), CANNY_HIP_MOTION_AFFINE = 2 (k = 3).
 *   Sampling: hypothesis h, 0 <= h < hypotheses, 1 <= hypotheses <= CANNY_HIP_MOTION_MAX_HYPOTHESES = 4096; it does not
 *     depend on the pair's position in the call.  s = (seed + 0x9E3779B9 * (h + 1)) mod 2^32; draw(n):
 *     s = (s * 1664525 + 1013904223) mod 2^32, the result is (s >> 16) % n.  i1 = draw(m); i2 = draw(m - 1), +1 if >= i1;
 *     i3 = draw(m - 2), +1 if >= min(i1, i2), then +1 if >= max(i1, i2).  Only the first k indices are drawn.  m < k: no
 *     model for this pair.
 *   Hypothesis, exact integers; q1, q1' the first sample.  TRANSLATION: D = 1, M = I.  SIMILARITY, d = q2 - q1,
 *     d' = q2' - q1': D = dx^2 + dy^2, A = dx dx' + dy dy', B = dx dy' - dy dx', M = [[A, -B], [B, A]].  AFFINE, e = q2 - q1,
 *     f = q3 - q1, e', f' likewise: D = ex fy - ey fx, M11 = e'x fy - f'x ey, M12 = f'x ex - e'x fx, M21 = e'y fy - f'y ey,
 *     M22 = f'y ex - e'y fx.  D == 0 makes the hypothesis invalid.
 *   Inlier test: r = D (c' - q1') - M (c - q1); c is an inlier iff 256 (rx^2 + ry^2) <= thr_q4^2 D^2; thr_q4 in 1/16 px,
 *     0 <= thr_q4 <= 4095.  |D| <= 2^33, |M| <= 2^34, |r| < 2^53: both sides fit unsigned 128 bits, the comparison is exact.
 *   Best hypothesis: the valid h with the most inliers, ties to the smallest h.  None: the "model" bit is clear and the
 *     inlier flags of all correspondences are 0.
 *   Refit over the n inliers of the best hypothesis: 64-bit sums Sx, Sy, Sx', Sy', Sxx, Sxy, Syy, Sxx', Sxy', Syx', Syy';
 *     C(ab) = n Sab - Sa Sb, |C| <= n^2 2^30 <= 2^54; fl = floor toward -inf.  TRANSLATION: a = [[65536, 0], [0, 65536]].
 *     SIMILARITY: Dn = Cxx + Cyy, a11 = a22 = fl(65536 (Cxx' + Cyy') / Dn), a21 = fl(65536 (Cxy' - Cyx') / Dn),
 *     a12 = -a21.  AFFINE: det = Cxx Cyy - Cxy^2, a11 = fl(65536 (Cxx' Cyy - Cyx' Cxy) / det),
 *     a12 = fl(65536 (Cyx' Cxx - Cxx' Cxy) / det), a21, a22 the same with y' for x'.  Every numerator times 65536 stays under
 *     2^126.  Dn or det <= 0, or any |a_ij| > 2^24: the "refit" bit is clear and words 4..11 are zero.  Then
 *     tx = fl((65536 Sx' - a11 Sx - a12 Sy) / n), ty likewise.  Residual per inlier: ex = 65536 x' - (a11 x + a12 y + tx),
 *     gx = ex >> 8 (arithmetic), clamped to +-2^24, gy likewise; word 10 is the sum of gx^2 + gy^2, word 11 its maximum.
 *   Record, CANNY_HIP_MOTION_WORDS = 16 long long per pair: 0 flags (bit 0 model, bit 1 refit); 1 m; 2 inliers; 3 best h
 *     (-1 if none); 4..9 a11, a12, tx, a21, a22, ty (Q16, query -> train); 10, 11 the residual words; 12..14 i1, i2, i3 as
 *     slot indices i of the query (-1 unused); 15 D.  Every pair writes all 16 words.
 *   Inlier flags: [n_pairs][stride_q] int: 1 an inlier of the best hypothesis, 0 a correspondence that is not, -1 a slot
 *     that is no correspondence; slots past the query count are not written.
 *   Statuses: bad ranges, NULL mandatory pointers, record buffers that are not 8-byte aligned, pair indices outside the
 *     sets: CANNY_HIP_ERR_INVALID; over a documented limit (a stride > 4096, hypotheses > 4096, more than 65535 frames,
 *     more than CANNY_HIP_MATCH_MAX_PAIRS pairs): CANNY_HIP_ERR_UNSUPPORTED; both before anything is queued, nothing is
 *     written.
 * Memory: the workspace holds the pairs, per (pair, query slot) 12 bytes and per (pair, hypothesis) one int.
 * The three parts are timed by canny_hip_motion_profile_get (CANNY_HIP_MOTION_PART_*); with "profile_stage_mask" they go by
 *   bit 30 like every part behind the polygons.
 * Not covered -- follow-ups: homography (8 degrees of freedom need wider than 128-bit exact arithmetic or another rule);
 * re-selecting the inliers after the refit (LO-RANSAC); a two-frame grammar of Main; motion through the batch pipeline or
 * the multi-GPU sharder. */
#define CANNY_HIP_MOTION_WORDS 16
#define CANNY_HIP_MOTION_MAX_HYPOTHESES 4096
enum canny_hip_motion_model {
    CANNY_HIP_MOTION_TRANSLATION = 0,
    CANNY_HIP_MOTION_SIMILARITY = 1,
    CANNY_HIP_MOTION_AFFINE = 2
};
enum canny_hip_motion_part {
    CANNY_HIP_MOTION_PART_GATHER = 0, /* the correspondences of every pair, compacted in query order */
    CANNY_HIP_MOTION_PART_SCORE = 1,  /* the inlier count of every (pair, hypothesis) */
    CANNY_HIP_MOTION_PART_REFIT = 2,  /* best hypothesis, inlier flags, refit, residuals, the record */
    CANNY_HIP_MOTION_PARTS = 3
};
/* pairs is a HOST array of 2 * n_pairs ints (q frame, t frame); every other pointer is a device pointer.  d_matches:
 * n_pairs * stride_q * 4 ints as the matcher wrote them; d_motion: n_pairs * 16 long long; d_inlier: n_pairs * stride_q
 * ints, may be NULL.  The two sets may be the same buffers.  Asynchronous. */
int canny_hip_dev_estimate_motion(canny_hip_ctx *ctx, const long long *d_q_corners, const int *d_q_counts, int n_q_frames,
                                  int stride_q, const long long *d_t_corners, const int *d_t_counts, int n_t_frames,
                                  int stride_t, const int *pairs, int n_pairs, const int *d_matches, int model, int thr_q4,
                                  int hypotheses, unsigned seed, long long *d_motion, int *d_inlier);
/* Host-only, needs no device: the rule on ONE pair of host record sets (n_q, n_t records of 4 long long; matches n_q * 4
 * ints).  motion receives 16 words, inlier (may be NULL) n_q ints.  0 <= n_q, n_t <= 4096. */
int canny_hip_estimate_motion(const long long *q_corners, int n_q, const long long *t_corners, int n_t, const int *matches,
                              int model, int thr_q4, int hypotheses, unsigned seed, long long *motion, int *inlier);
/* Host buffers, synchronous: canny, the corners, their descriptors, the matching over `pairs` (HOST, frames of this batch)
 * and the motion of every pair, all on the device; only motion (n_pairs * 16 long long) comes down and, where the pointer is
 * not NULL, corners (n_frames * corners_max * 4 long long, the filled slots) with counts (n_frames ints; both or neither),
 * matches (n_pairs * corners_max * 4 ints) and inlier (n_pairs * corners_max ints; of both, the slots below the query's
 * count). */
int canny_hip_canny_motion(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                           int max_val, int height, int width, int mode, int block, int k_q8, int quality_q16,
                           long long min_response, int min_dist, int corners_max, int desc_options, const int *pairs,
                           int n_pairs, int max_distance, int ratio_q8, int match_options, int model, int thr_q4,
                           int hypotheses, unsigned seed, long long *motion, long long *corners, int *counts, int *matches,
                           int *inlier);

/* ---- frame alignment: chain the motions and warp frames ----------------------------------------------------------------------
 * The motion records say how the camera moved between consecutive frames; this applies them.  The records of the pairs
 * (f, f + 1) are chained into one transform per frame, and u8 frames are warped by such transforms -- what
 * cv::warpAffine(..., WARP_INVERSE_MAP) answers -- on the GPU, on the context's stream, no host round trip, no atomics.  A
 * motion record is stored query -> train in Q16, which is exactly the output -> source map of an inverse warp: aligning frame
 * f + k onto frame f needs no matrix inversion.  All integers: the same bytes on every run and every machine.
 * tests/warp_rule.py restates both rules in numpy and plain Python ints, csrc/canny_warp_host.cpp in plain C++.
 * THE RULE:
 *   Transform record, CANNY_HIP_XFORM_WORDS = 8 long long per output frame: 0 flags (bit 0 usable); 1 the source frame index;
 *     2..7 a11, a12, tx, a21, a22, ty in Q16, in the order of words 4..9 of a motion record: output pixel (x, y) -> source
 *     position.  A record is USABLE iff bit 0 is set, every |a_ij| <= 2^24, |tx|, |ty| <= 2^36 and 0 <= word 1 < n_src.
 *     Callers may write such records themselves.
 *   Chain (compose): d_motion holds the motion records of the consecutive pairs (f, f + 1), f = first_frame .., as
 *     consecutive_pairs of the Python binding orders them; n_pairs + 1 records are written, record k maps the pixels of frame
 *     first_frame into frame first_frame + k: word 1 = first_frame + k.  T_0 = (65536, 0, 0, 0, 65536, 0), the identity.
 *     T_{k+1} = M_k o T_k, fl = floor toward -inf, m the motion's coefficients, p those of T_k:
 *       a_ij = fl((m_i1 p_1j + m_i2 p_2j) / 65536),   t_i = fl((m_i1 p_tx + m_i2 p_ty) / 65536) + m_ti.
 *     M_k is used only if its record has flag bits 0 and 1 (model and refit) and every |m_ij| <= 2^24, |m_ti| <= 2^36; if it
 *     fails, or the composed record exceeds these limits, this record and every later one gets flags 0 and zero coefficients
 *     (word 1 is still written).  Widths: the linear sums stay under 2^50 and the translation sums under 2^62, so signed 64
 *     bits suffice.  The rounding makes composition non-associative, so the rule is sequential: one lane walks the chain.
 *     0 <= n_pairs <= 65535, first_frame >= 0.
 *   Warp: source planes [n_src][src_h][src_w] u8, output planes [n_out][out_h][out_w] u8, one record per output frame.  For
 *     output pixel (x, y) of a frame with a usable record, exact integers, |X| < 2^41:
 *       X = a11 x + a12 y + tx,   Y = a21 x + a22 y + ty.
 *     CANNY_HIP_WARP_NEAREST = 0: sx = (X + 32768) >> 16, sy likewise (arithmetic shifts); the pixel is src[word 1][sy][sx] if
 *       that lies inside the source, otherwise `border`.
 *     CANNY_HIP_WARP_BILINEAR = 1: X8 = (X + 128) >> 8, ix = X8 >> 8, fx = X8 & 255, the same for y; four taps p00 = (iy, ix),
 *       p01 = (iy, ix + 1), p10 = (iy + 1, ix), p11 = (iy + 1, ix + 1), each the source byte if inside, else `border`
 *       (BORDER_CONSTANT);
 *       out = ((256 - fx)(256 - fy) p00 + fx (256 - fy) p01 + (256 - fx) fy p10 + fx fy p11 + 32768) >> 16.
 *       The weights are Q8, so the sum stays under 2^24 and the identity returns the input bytes.
 *     Valid bit: 1 iff every tap with a non-zero weight lies inside the source (NEAREST: the one tap); the identity is valid
 *       everywhere.  A record that is not usable: the whole frame is `border`, every valid bit 0.  Every output byte is
 *       written, and every valid byte (layout of canny_hip_dev_canny_bits: rows MSB-first, padded to bytes, pad bits 0).
 *   Limits: all four dimensions >= 1 and <= 32768, each plane < 2^31 pixels, at most 65535 frames on either side, 65535 pairs;
 *     above: CANNY_HIP_ERR_UNSUPPORTED.  Bad ranges (interp, border outside [0, 255], counts < 1), NULL mandatory pointers, a
 *     source and an output that overlap, record buffers that are not 8-byte aligned: CANNY_HIP_ERR_INVALID.  Both before
 *     anything is queued; nothing is written.
 *   The context option "warp_route" chooses how the taps are fetched: 0 automatic, 1 direct (gathered from global memory
 *     through the vector cache), 2 tiled (the source footprint of every 64 x 16 output tile -- the bounding box of the images
 *     of its four corners, one more row and column under BILINEAR, clipped to the source -- is staged in LDS with coalesced
 *     row loads where it fits CANNY_HIP_WARP_LDS_BYTES, and that tile alone falls back to the direct gather where it does
 *     not).  All routes give the same bytes.  Automatic is the direct route, except under BILINEAR for records with
 *     |a21| >= |a11| (a turn of 45 degrees or more), where it is the tiled one: where the measurement shows each ahead.
 * The two parts are timed by canny_hip_warp_profile_get (CANNY_HIP_WARP_PART_*); with "profile_stage_mask" they go by bit 30
 *   like every part behind the polygons.
 * Not covered -- follow-ups: inverting a model (anchors other than the first frame, trajectory smoothing); s16 or colour
 * planes, and warping the finished edge maps; bicubic interpolation; a grammar of Main (it takes one frame); alignment through
 * the batch pipeline or the multi-GPU sharder. */
#define CANNY_HIP_XFORM_WORDS 8
#define CANNY_HIP_WARP_LDS_BYTES 16384
enum canny_hip_warp_interp { CANNY_HIP_WARP_NEAREST = 0, CANNY_HIP_WARP_BILINEAR = 1 };
enum canny_hip_warp_part {
    CANNY_HIP_WARP_PART_COMPOSE = 0, /* the chain of the motion records */
    CANNY_HIP_WARP_PART_WARP = 1,    /* the warp of the frames */
    CANNY_HIP_WARP_PARTS = 2
};
/* d_motion: n_pairs * 16 long long as the motion estimate wrote them (may be NULL if n_pairs == 0); d_xforms receives
 * (n_pairs + 1) * 8 long long.  Asynchronous. */
int canny_hip_dev_compose_motion(canny_hip_ctx *ctx, const long long *d_motion, int n_pairs, int first_frame,
                                 long long *d_xforms);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_compose_motion(const long long *motion, int n_pairs, int first_frame, long long *xforms);
/* d_xforms: n_out * 8 long long; d_out: n_out * out_h * out_w bytes; d_valid_bits: n_out * out_h * ((out_w + 7) / 8)
 * bytes, may be NULL.  Asynchronous. */
int canny_hip_dev_warp_frames(canny_hip_ctx *ctx, const unsigned char *d_src, int n_src, int src_h, int src_w,
                              const long long *d_xforms, int n_out, int out_h, int out_w, int interp, int border,
                              unsigned char *d_out, unsigned char *d_valid_bits);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_warp_frames(const unsigned char *src, int n_src, int src_h, int src_w, const long long *xforms, int n_out,
                          int out_h, int out_w, int interp, int border, unsigned char *out, unsigned char *valid_bits);
/* Host buffers, synchronous: canny, the corners, their descriptors, the matching and the motion over the consecutive pairs
 * (f, f + 1), the chain from frame 0 and the warp of the INPUT gray frames to frame 0's geometry, all on the device.  aligned
 * (n_frames * height * width bytes) and xforms (n_frames * 8 long long) come down and, where the pointer is not NULL, motion
 * ((n_frames - 1) * 16 long long) and valid_bits (n_frames * height * ((width + 7) / 8) bytes).  n_frames == 1 returns the
 * frame itself with an identity record. */
int canny_hip_canny_align(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                          int height, int width, int mode, int block, int k_q8, int quality_q16, long long min_response,
                          int min_dist, int corners_max, int desc_options, int max_distance, int ratio_q8, int match_options,
                          int model, int thr_q4, int hypotheses, unsigned seed, int interp, int border,
                          unsigned char *aligned, long long *xforms, long long *motion, unsigned char *valid_bits);

/* ---- temporal fusion of aligned frames and change masks -------------------------------------------------------------------
 * What the alignment is for: a per-pixel reduction over the time axis of a stack of u8 frames that honours the valid bits the
 * warp writes (average, median background, extremes), and a per-frame change mask against the fused plane, written in the
 * packed bit-map layout that canny_hip_dev_components_bits, _edt_bits, _contours_bits and _points_from_bits take -- so a
 * video batch goes to "what moved in each frame, as labelled components" on one stream, without a download.  All integers, no
 * floats, no atomics whose order could matter: the same bytes on every run and every machine.  tests/fuse_rule.py restates
 * the rule in numpy and Python ints, csrc/canny_fuse_host.cpp in plain C++.
 * THE RULE:
 *   Fuse.  frames [n_frames][h][w] u8; valid_bits [n_frames][h][(w + 7) / 8], rows MSB-first (the layout the warp writes);
 *     the PAD BITS OF THE INPUT ARE IGNORED; valid_bits == NULL means every pixel is valid.
 *     Windows: window g holds the frames g * group_step .. g * group_step + group_len - 1;
 *       n_groups = (n_frames - group_len) / group_step + 1;  1 <= group_len <= min(n_frames, 255), group_step >= 1.
 *       group_step = group_len: disjoint groups; group_step = 1: a sliding window; group_len = n_frames: one background.
 *       Frames behind the last window belong to no window and are not read.
 *     Per output pixel: c = the number of valid frames of the window (<= 255: a byte), v_0 <= .. <= v_{c-1} their values
 *       sorted, s their sum (<= 255 * 255 = 65025).
 *       CANNY_HIP_FUSE_MEAN   = 0: (2 s + c) / (2 c), integer division: rounds half up (2 s + c <= 130305 < 2^17)
 *       CANNY_HIP_FUSE_MEDIAN = 1: v_{(c - 1) >> 1}, the lower median
 *       CANNY_HIP_FUSE_MIN    = 2: v_0
 *       CANNY_HIP_FUSE_MAX    = 3: v_{c-1}
 *     If c < min_count (1 <= min_count <= 255) the pixel is `fill` (0..255).  fused [n_groups][h][w] u8 is always written in
 *     full; count [n_groups][h][w] u8 receives c -- the true count, also where `fill` was written -- if the pointer is not
 *     NULL.
 *   Change mask.  Frame f is compared with background plane f / frames_per_background (frames_per_background >= 1;
 *     n_background = ceil(n_frames / frames_per_background); frames_per_background >= n_frames: one background for all
 *     frames; frames_per_background = group_len pairs with disjoint groups).  Bit (f, y, x) is 1 iff
 *       the frame's valid bit is set, or valid_bits is NULL;  and
 *       bg_count is NULL or bg_count[f / frames_per_background][y][x] >= min_count;  and
 *       |frame - background| > thr, 0 <= thr <= 255.
 *     mask_bits [n_frames][h][(w + 7) / 8]: the layout of canny_hip_dev_canny_bits -- rows MSB-first, padded to bytes, PAD
 *     BITS WRITTEN 0, every byte written.  changed[f] (one long long per frame, the pointer may be NULL) is the number of set
 *     bits of frame f: an integer sum, so it does not depend on order; it is fully written by the call, and not touched by a
 *     refused one.
 *   Limits: h, w in 1..32768, a plane < 2^31 pixels, at most 65535 frames; above: CANNY_HIP_ERR_UNSUPPORTED.  Bad ranges
 *     (group_len, group_step, op, fill, min_count, frames_per_background, thr, counts < 1), NULL mandatory pointers, an output
 *     that overlaps an input or another output, a `changed` buffer that is not 8-byte aligned: CANNY_HIP_ERR_INVALID.  Both
 *     before anything is queued; nothing is written.
 *   Kernels (csrc/canny_fuse.hip): one workgroup of 256 per 64 x 16 output tile and trip of a grid capped at 4096; a lane owns
 *     four adjacent pixels, loads one 32-bit word per frame and stores one word (byte paths where w is no multiple of 4, the
 *     buffer is not 4-byte aligned or the run crosses the row end); every output byte has one writer.  The mean's division
 *     is a multiplication: q = (n * M(c)) >> 32 with n = 2 s + c and M(c) = floor((2^32 - 1) / (2 c)) + 1 from a table of 256
 *     words in LDS; M(c) * 2c = 2^32 + e with 0 <= e < 2c <= 510, and n * e < 2^27 < 2^32, so q is the exact quotient for every
 *     (s, c) of the domain -- canny_hip_selftest_fuse_mean runs that helper over all of them on the device.
 *   The context option "fuse_route" chooses how the MEDIAN is selected: 0 automatic, 1 registers (group_len <= 32: the window
 *     is read once and stays in registers as 16-bit lanes, 0x100 + v for an invalid sample so that it sorts behind every valid
 *     one; an odd-even merge sorting network of packed 16-bit min/max over 8, 16 or 32 slots, two pixels an instruction; the
 *     rank is picked by compares, no indexed registers), 2 passes (any group_len: a count pass and eight passes of a binary
 *     radix select that re-read the window).  Route 1 with group_len > 32 runs the passes.  All routes give the same bytes;
 *     the other ops take one pass under every route.
 * The two parts are timed by canny_hip_fuse_profile_get (CANNY_HIP_FUSE_PART_*); with "profile_stage_mask" they go by bit 30
 *   like every part behind the polygons.
 * Not covered -- follow-ups: colour or s16 planes; a running background with exponential update; morphology on the mask; a
 * grammar of Main; fusion through the batch pipeline or the multi-GPU sharder. */
#define CANNY_HIP_FUSE_MAX_GROUP 255
#define CANNY_HIP_FUSE_MEAN_ROW 65026 /* canny_hip_selftest_fuse_mean: cells of a row, s = 0 .. 255 * 255 */
enum canny_hip_fuse_op {
    CANNY_HIP_FUSE_MEAN = 0,
    CANNY_HIP_FUSE_MEDIAN = 1,
    CANNY_HIP_FUSE_MIN = 2,
    CANNY_HIP_FUSE_MAX = 3
};
enum canny_hip_fuse_part {
    CANNY_HIP_FUSE_PART_FUSE = 0, /* the reduction over the windows */
    CANNY_HIP_FUSE_PART_MASK = 1, /* the change masks and their counts */
    CANNY_HIP_FUSE_PARTS = 2
};
/* d_frames: n_frames * h * w bytes; d_valid_bits: n_frames * h * ((w + 7) / 8) bytes or NULL; d_fused and d_count (may be
 * NULL): n_groups * h * w bytes.  Asynchronous. */
int canny_hip_dev_fuse_frames(canny_hip_ctx *ctx, const unsigned char *d_frames, const unsigned char *d_valid_bits,
                              int n_frames, int h, int w, int group_len, int group_step, int op, int fill, int min_count,
                              unsigned char *d_fused, unsigned char *d_count);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_fuse_frames(const unsigned char *frames, const unsigned char *valid_bits, int n_frames, int h, int w,
                          int group_len, int group_step, int op, int fill, int min_count, unsigned char *fused,
                          unsigned char *count);
/* d_background and d_bg_count (may be NULL): ceil(n_frames / frames_per_background) * h * w bytes; d_mask_bits: n_frames * h *
 * ((w + 7) / 8) bytes; d_changed: n_frames long long, may be NULL.  Asynchronous. */
int canny_hip_dev_change_mask(canny_hip_ctx *ctx, const unsigned char *d_frames, const unsigned char *d_valid_bits,
                              int n_frames, int h, int w, const unsigned char *d_background,
                              const unsigned char *d_bg_count, int frames_per_background, int thr, int min_count,
                              unsigned char *d_mask_bits, long long *d_changed);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_change_mask(const unsigned char *frames, const unsigned char *valid_bits, int n_frames, int h, int w,
                          const unsigned char *background, const unsigned char *bg_count, int frames_per_background, int thr,
                          int min_count, unsigned char *mask_bits, long long *changed);
/* Host buffers, synchronous: the whole chain of canny_hip_canny_align on the device (its arguments up to `border`), then all
 * n_frames aligned frames fused into one plane (group_len = n_frames, so n_frames <= 255; more: CANNY_HIP_ERR_INVALID) with
 * the alignment's valid bits, then the change masks of the aligned frames against that plane (with its counts and
 * min_count).  background (height * width bytes) and xforms (n_frames * 8 long long) come down and, where the pointer is not
 * NULL, count (height * width bytes), mask_bits (n_frames * height * ((width + 7) / 8) bytes) and changed (n_frames long
 * long).  The aligned frames and their valid bits stay in a workspace of the context. */
int canny_hip_canny_background(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val,
                               int max_val, int height, int width, int mode, int block, int k_q8, int quality_q16,
                               long long min_response, int min_dist, int corners_max, int desc_options, int max_distance,
                               int ratio_q8, int match_options, int model, int thr_q4, int hypotheses, unsigned seed,
                               int interp, int border, int op, int fill, int min_count, int thr, unsigned char *background,
                               unsigned char *count, unsigned char *mask_bits, long long *changed, long long *xforms);

/* ---- binary morphology on packed bit maps -------------------------------------------------------------------------------
 * The operator that maps a bit map to a bit map: erode, dilate, open, close, gradient, top hat and black hat -- what
 * cv::erode / cv::dilate / cv::morphologyEx answer on a binary image -- on the packed layout of canny_hip_dev_canny_bits and
 * canny_hip_dev_change_mask, which canny_hip_dev_components_bits, _edt_bits, _contours_bits and _points_from_bits take as it
 * is: a change mask is cleaned of salt and pepper, an edge map has its one-pixel breaks closed, on the context's stream,
 * without a download.  All bit operations: the same bytes on every run and every machine.  tests/morph_rule.py restates the
 * rule in numpy, csrc/canny_morph_host.cpp in plain C++.
 * THE RULE:
 *   Bit maps.  [n_frames][h][(w + 7) / 8] bytes, rows MSB-first.  THE PAD BITS OF THE INPUT ARE IGNORED: a column >= w is
 *     outside the frame, whatever the byte holds.  THE PAD BITS OF THE OUTPUT ARE WRITTEN 0, and every output byte is written.
 *   Element.  kw, kh odd, 1..31 (CANNY_HIP_MORPH_MAX_EXTENT); rows[kh] unsigned words; bit i (LSB = 0) of rows[j] is the offset
 *     (dx, dy) = (i - kw / 2, j - kh / 2).  Bits at or above kw must be 0 and at least one bit must be set, otherwise
 *     CANNY_HIP_ERR_INVALID.  The centre need not be set.  canny_hip_morph_element fills rows for a shape:
 *       CANNY_HIP_MORPH_RECT    = 0: all bits set
 *       CANNY_HIP_MORPH_CROSS   = 1: the centre row and the centre column
 *       CANNY_HIP_MORPH_ELLIPSE = 2: dx^2 ry^2 + dy^2 rx^2 <= rx^2 ry^2 with rx = kw / 2, ry = kh / 2; all bits if rx or ry is
 *         0.  For kw = kh = 2 r + 1 this is skimage.morphology.disk(r); 3 x 3 gives the cross.
 *   Primitives, B the set of the element's offsets:
 *       ERODE : out(p) = AND over b in B of in(p + b)
 *       DILATE: out(p) = OR  over b in B of in(p - b)   -- the Minkowski sum: the element reflected
 *     These are scipy.ndimage.binary_erosion / binary_dilation with structure = B, and cv::erode / cv::dilate for symmetric
 *     elements.
 *   Border.  What a pixel outside the frame reads as: CANNY_HIP_MORPH_BORDER_ZERO = 0 reads 0, _ONE = 1 reads 1, _NEUTRAL = 2
 *     reads 1 in an erosion step and 0 in a dilation step (OpenCV's default: the outside constrains nothing).
 *   Ops, iterations in 1..16 (CANNY_HIP_MORPH_MAX_ITERATIONS):
 *       CANNY_HIP_MORPH_ERODE = 0, _DILATE = 1: the primitive `iterations` times in sequence
 *       CANNY_HIP_MORPH_OPEN  = 2: `iterations` erosions, then `iterations` dilations
 *       CANNY_HIP_MORPH_CLOSE = 3: `iterations` dilations, then `iterations` erosions
 *       CANNY_HIP_MORPH_GRADIENT = 4: DILATE & ~ERODE;  _TOPHAT = 5: in & ~OPEN;  _BLACKHAT = 6: CLOSE & ~in -- inside the frame
 *     With the reflected dilation and the neutral border OPEN is idempotent and anti-extensive and CLOSE idempotent and
 *     extensive, for every element.
 *   Counts.  counts may be NULL; otherwise n_frames long long, 8-byte aligned: the set bits of each output frame, an integer
 *     sum (no order to depend on), zeroed on the stream inside the call, fully written by it and not touched by a refused one.
 *   Limits: h, w in 1..32768, a plane < 2^31 pixels, at most 65535 frames; above: CANNY_HIP_ERR_UNSUPPORTED.  Bad enum values,
 *     bad ranges, NULL mandatory pointers, a bad element, a misaligned counts buffer, an output that overlaps the input (there
 *     is no in-place form) or the counts: CANNY_HIP_ERR_INVALID.  Both before anything is queued; nothing is written.
 *   Kernels (csrc/canny_morph.hip): one launch per primitive step; a workgroup of 256 per tile of 8 x 64-bit words x 64 rows and
 *     trip of a grid capped at 4096.  Rows become LSB-first 64-bit words in LDS with the outside value put in where the words
 *     are formed; a horizontal offset is a shift with the carry from the neighbouring word, a run of L set element bits costs
 *     O(log L) shifts by doubling, a vertical offset is another row's word.  The context option "morph_route": 0 automatic,
 *     1 general (per element row its runs), 2 separable (full rectangles: the horizontal run, then the vertical run by doubling
 *     in LDS; any other element runs the general route).  All routes give the same bytes.  Sequential steps go through one
 *     context workspace of two maps (and, for GRADIENT, the output buffer); the final combination, the pad bits and the counts
 *     belong to the last step's kernel.
 * Not covered -- follow-ups: grey-level morphology on u8 planes; hit-or-miss (thinning: see below); elements wider than 31; morphology
 * through the batch pipeline or the multi-GPU sharder; a grammar of Main for fusion and change masks. */
#define CANNY_HIP_MORPH_MAX_EXTENT 31
#define CANNY_HIP_MORPH_MAX_ITERATIONS 16
enum canny_hip_morph_op {
    CANNY_HIP_MORPH_ERODE = 0,
    CANNY_HIP_MORPH_DILATE = 1,
    CANNY_HIP_MORPH_OPEN = 2,
    CANNY_HIP_MORPH_CLOSE = 3,
    CANNY_HIP_MORPH_GRADIENT = 4,
    CANNY_HIP_MORPH_TOPHAT = 5,
    CANNY_HIP_MORPH_BLACKHAT = 6
};
enum canny_hip_morph_shape {
    CANNY_HIP_MORPH_RECT = 0,
    CANNY_HIP_MORPH_CROSS = 1,
    CANNY_HIP_MORPH_ELLIPSE = 2
};
enum canny_hip_morph_part {
    CANNY_HIP_MORPH_PART_STEPS = 0, /* all primitive steps of a call, with the zeroing of the counts */
    CANNY_HIP_MORPH_PARTS = 1
};
enum canny_hip_morph_border {
    CANNY_HIP_MORPH_BORDER_ZERO = 0,
    CANNY_HIP_MORPH_BORDER_ONE = 1,
    CANNY_HIP_MORPH_BORDER_NEUTRAL = 2
};
/* d_bits, d_out_bits: n_frames * h * ((w + 7) / 8) bytes, any byte address; rows: kh words of HOST memory, copied at call
 * time; d_counts: n_frames long long or NULL.  Asynchronous, on the context's stream. */
int canny_hip_dev_morph_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int h, int w, int op,
                             const unsigned *rows, int kw, int kh, int border, int iterations, unsigned char *d_out_bits,
                             long long *d_counts);
/* The same operator on the strong bit-plane that the preceding dev_canny of the same n_frames, h, w left in the context (any
 * canny_hip_dev_canny* call; another geometry, or none yet: CANNY_HIP_ERR_INVALID).  The plane is the finished map for
 * max_val <= 255; it is only read, so the call may be repeated and mixed with the other analysis calls.  Asynchronous. */
int canny_hip_dev_canny_morph(canny_hip_ctx *ctx, int n_frames, int h, int w, int op, const unsigned *rows, int kw, int kh,
                              int border, int iterations, unsigned char *d_out_bits, long long *d_counts);
/* Host buffers, synchronous: upload, canny, the operator on the finished map; only out_bits (n_frames * height * ((width + 7)
 * / 8) bytes) and, where the pointer is not NULL, counts come down. */
int canny_hip_canny_morph(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, float sigma, int min_val, int max_val,
                          int height, int width, int op, const unsigned *rows, int kw, int kh, int border, int iterations,
                          unsigned char *out_bits, long long *counts);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_morph_bits(const unsigned char *bits, int n_frames, int h, int w, int op, const unsigned *rows, int kw, int kh,
                         int border, int iterations, unsigned char *out_bits, long long *counts);
/* Host-only: rows[kh] of a canny_hip_morph_shape; kw, kh odd, 1..31. */
int canny_hip_morph_element(int shape, int kw, int kh, unsigned *rows);

/* ---- binarization: gray planes to packed bit maps ------------------------------------------------------------------------
 * The operator in front of every stage that takes a packed bit map (components, contours, polygons, shapes, curves, the
 * distance transform, chamfer matching, point lists, binary morphology): what cv::threshold(THRESH_BINARY[_INV]),
 * cv::threshold(THRESH_OTSU) and cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) answer, on u8 planes as they lie on the
 * device (frames, warped frames, fused backgrounds, the smoothed plane dev_canny left in the context), on the context's
 * stream, without a download.  All integers: the same bytes on every run and every machine.  tests/binarize_rule.py restates
 * the rule in numpy and Python ints, csrc/canny_binarize_host.cpp in plain C++.
 * THE RULE:
 *   Input [n_frames][h][w] u8.  Output [n_frames][h][(w + 7) / 8] bytes, rows MSB-first, the layout of
 *     canny_hip_dev_canny_bits.  THE PAD BITS ARE WRITTEN 0, and every output byte is written.
 *   For a pixel of value v the bit is cond(v) XOR invert, invert in {0, 1}: 0 is THRESH_BINARY, 1 THRESH_BINARY_INV.  The XOR
 *     applies inside the frame only.
 *   CANNY_HIP_BIN_FIXED = 0: cond = v > thr, thr = thr_or_c in -1..255, the same for all frames; thr = -1 sets every pixel.
 *   CANNY_HIP_BIN_OTSU = 1: cond = v > t[f], every frame with its own t[f] from its 256-bin histogram hist (thr_or_c is
 *     ignored).  With N = sum hist, S = sum i hist[i] and, for t = 0..255,
 *       w0 = sum_{i <= t} hist[i], s0 = sum_{i <= t} i hist[i], w1 = N - w0, s1 = S - s0, d = w1 s0 - s1 w0,
 *       score(t) = 0 if w0 w1 == 0, else floor(d^2 / (w0 w1)),
 *     t[f] is the SMALLEST t with the LARGEST score; a flat frame gets 0.  This is Otsu's between-class variance times the
 *     frame's constant N^2, floored.  Domain: frames of at most 2^26 pixels (|d| < 2^58, d^2 < 2^116, w0 w1 <= 2^50: a 128-bit
 *     product and a 128-by-64 division); above: CANNY_HIP_ERR_UNSUPPORTED.
 *   CANNY_HIP_BIN_ADAPTIVE_MEAN = 2: cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) with the build-dependent float mean
 *     replaced by integers.  Window kw x kh, both odd, 3..255 (CANNY_HIP_BIN_MAX_EXTENT), A = kw kh; offset c = thr_or_c in
 *     -255..255.  S = the sum of the window centred on the pixel, coordinates clamped to the frame (BORDER_REPLICATE,
 *     OpenCV's border there); S <= 255 * 255 * 255 < 2^24.  m = (2 S + A) / (2 A), the mean rounded half up, and
 *     cond = v > m - c.  EQUIVALENTLY, WITHOUT A DIVISION: cond = 2 S < A (2 (v + c) - 1) -- among integers v > m - c is
 *     m <= v + c - 1, floor(x / k) <= n is x < k (n + 1) for k > 0, so it is 2 S + A < 2 A (v + c); the kernels compute this
 *     form, the host the other.  kw and kh are ignored by the other methods.
 *   counts may be NULL; otherwise n_frames long long, 8-byte aligned: the set bits of each output frame, an integer sum (no
 *     order to depend on), zeroed on the stream inside the call, fully written by it and not touched by a refused one.
 *   thresholds may be NULL; otherwise n_frames ints: OTSU t[f], FIXED thr, ADAPTIVE_MEAN c.
 *   Limits: h, w in 1..32768, a plane < 2^31 pixels, at most 65535 frames (OTSU: a frame <= 2^26 pixels); above:
 *     CANNY_HIP_ERR_UNSUPPORTED.  Bad enum values, bad ranges, NULL mandatory pointers, a misaligned counts buffer, buffers
 *     that overlap: CANNY_HIP_ERR_INVALID.  Both before anything is queued; nothing is written.
 *   Kernels (csrc/canny_binarize.hip).  FIXED and OTSU: one map kernel, the frame's threshold from a device array (FIXED
 *     fills it on the stream), a lane per output byte, 256 bytes of one frame per workgroup and trip of a grid capped at 4096,
 *     the counts by wave reduction and one atomic add per workgroup and frame.  OTSU: the u8 histogram kernel of the automatic
 *     hysteresis thresholds, then one workgroup per frame (two block prefix sums, a candidate t per lane with a restoring
 *     division, arg-max with ties to the smaller t).  ADAPTIVE_MEAN, the context option "binarize_route": 0 automatic,
 *     1 straightforward (every lane sums its windows from global memory: the cross-check), 2 marching (a wave per strip of 512
 *     useful columns and segment of rows: vertical running sums of the staged columns in registers, the horizontal window
 *     from a prefix sum through LDS, the bits by ballot).  Both routes give the same bytes.
 * Not covered -- follow-ups: Gaussian-weighted adaptive thresholds; Sauvola and Niblack; a valid-bits input; s16 planes;
 * binarization through the batch pipeline or the multi-GPU sharder. */
#define CANNY_HIP_BIN_MAX_EXTENT 255
enum canny_hip_bin_method {
    CANNY_HIP_BIN_FIXED = 0,
    CANNY_HIP_BIN_OTSU = 1,
    CANNY_HIP_BIN_ADAPTIVE_MEAN = 2
};
enum canny_hip_bin_part {
    CANNY_HIP_BIN_PART_HISTOGRAM = 0, /* OTSU: the zeroing of the histograms and the histogram kernel */
    CANNY_HIP_BIN_PART_SELECT = 1,    /* OTSU: the threshold of every frame */
    CANNY_HIP_BIN_PART_MAP = 2,       /* every method: the kernel that writes the bits, with the zeroing of the counts */
    CANNY_HIP_BIN_PARTS = 3
};
/* d_plane: n_frames * h * w bytes, any byte address, or NULL: the smoothed plane that the preceding dev_canny of the same
 * n_frames, h, w left in the context (any canny_hip_dev_canny* call; another geometry, or none yet: CANNY_HIP_ERR_INVALID;
 * the plane is only read).  d_out_bits: n_frames * h * ((w + 7) / 8) bytes, any byte address; d_counts: n_frames long long or
 * NULL; d_thresholds: n_frames ints or NULL.  Asynchronous, on the context's stream. */
int canny_hip_dev_binarize(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int method,
                           int thr_or_c, int kw, int kh, int invert, unsigned char *d_out_bits, long long *d_counts,
                           int *d_thresholds);
/* Host buffers, synchronous: upload, the operator; only out_bits and, where the pointers are not NULL, counts and thresholds
 * come down. */
int canny_hip_binarize_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int method,
                             int thr_or_c, int kw, int kh, int invert, unsigned char *out_bits, long long *counts,
                             int *thresholds);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_binarize(const unsigned char *imgs, int n_frames, int h, int w, int method, int thr_or_c, int kw, int kh,
                       int invert, unsigned char *out_bits, long long *counts, int *thresholds);
/* Host-only: Otsu's threshold of the rule for a histogram of the caller's: 256 bins, at most 2^26 samples in all
 * (CANNY_HIP_ERR_UNSUPPORTED above). */
int canny_hip_otsu_from_histogram(const unsigned long long *hist256, int *t);

/* ---- thinning of packed bit maps to one-pixel skeletons --------------------------------------------------------------------
 * The step between "bits" and the stages that assume strokes one pixel wide (the curve linker, the polygons, the line and
 * circle fits): what cv::ximgproc::thinning and skimage.morphology.thin answer, on the packed layout of
 * canny_hip_dev_canny_bits, on the context's stream, without a download.  A binarized frame or a change mask goes
 * binarize -> morph -> thin -> curves on the device.  All bit operations: the same bytes on every run, route and machine.
 * tests/thin_rule.py restates the rule in numpy, csrc/canny_thin_host.cpp pixel by pixel in plain C++.
 * THE RULE:
 *   Bit maps [n_frames][h][(w + 7) / 8] bytes, rows MSB-first.  THE PAD BITS OF THE INPUT ARE IGNORED, THE PAD BITS OF THE
 *     OUTPUT ARE WRITTEN 0, every output byte is written, EVERYTHING OUTSIDE THE FRAME READS 0, frames never see each other.
 *   Neighbours of a pixel P1 = (y, x): P2 = (y-1, x), P3 = (y-1, x+1), P4 = (y, x+1), P5 = (y+1, x+1), P6 = (y+1, x),
 *     P7 = (y+1, x-1), P8 = (y, x-1), P9 = (y-1, x-1).
 *   One full iteration is sub-iteration 0 on the whole frame, then sub-iteration 1 on the result; within a sub-iteration
 *     every pixel decides from the same input map (fully parallel).
 *   CANNY_HIP_THIN_ZHANGSUEN = 0: a set P1 is deleted iff B = P2 + .. + P9 is in 2..6, A = 1 -- A the number of i with
 *     ring[i] = 0 and ring[i+1] = 1 over the cyclic ring P2, P3, .., P9, P2 -- and
 *       sub-iteration 0: P2 P4 P6 = 0 and P4 P6 P8 = 0;   sub-iteration 1: P2 P4 P8 = 0 and P2 P6 P8 = 0.
 *     ZHANGSUEN DOES NOT PRESERVE COMPONENTS: it erases a 2 x 2 square and reduces a two-pixel-wide diagonal to one pixel.
 *   CANNY_HIP_THIN_GUOHALL = 1: a set P1 is deleted iff C = 1, 2 <= min(N1, N2) <= 3 and m = 0, with
 *       C  = (!P2 & (P3 | P4)) + (!P4 & (P5 | P6)) + (!P6 & (P7 | P8)) + (!P8 & (P9 | P2)),
 *       N1 = (P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8),   N2 = (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9),
 *       sub-iteration 0: m = (P6 | P7 | !P9) & P8;   sub-iteration 1: m = (P2 | P3 | !P5) & P4.
 *     It kept the number of 8-connected components on every map tried and is what the examples and Main default to.
 *   Stopping.  D = the number of full iterations, from the start, that delete at least one pixel (finite).  max_iterations =
 *     k >= 1: the output is the map after min(k, D) full iterations; max_iterations = 0: after D, the fixed point.
 *     max_iterations in 0..16384 (CANNY_HIP_THIN_MAX_ITERATIONS).
 *   info may be NULL; otherwise 4 long long per frame, 8-byte aligned: [0] the set bits of the output frame, [1] iterations =
 *     min(k, D), or D for k = 0, [2] the pixels deleted = the set bits of the input inside the frame minus [0], [3] converged =
 *     1 if k = 0 or D < k, else 0 (a run cut at exactly D reports 0: no iteration proved the fixed point).  Zeroed on the
 *     stream inside the call, fully written by it and not touched by a refused one.
 *   Facts (tests/test_thin_rule.py): the output is a subset of the input and idempotent; a bar of thickness t takes t / 2
 *     iterations and leaves one row; an all-set 33 x 47 frame takes 16; GUOHALL keeps 1 pixel of the 2 x 2 square and 13 of the
 *     diagonal's 23.  No byte equality with OpenCV at the frame border is claimed: the rule above is the specification.
 *   Limits: h, w in 1..32768, a plane < 2^31 pixels, at most 65535 frames; above: CANNY_HIP_ERR_UNSUPPORTED.  Bad enum values,
 *     bad ranges, NULL mandatory pointers, a misaligned info buffer, an output that overlaps the input or the info (there is
 *     no in-place form): CANNY_HIP_ERR_INVALID.  Both before anything is queued; nothing is written.
 *   Kernels (csrc/canny_thin.hip): a workgroup of 256 per tile of 8 x 64-bit words x 64 rows of a grid capped at 4096, rows
 *     staged in LDS as whole words with the outside zero put in where the words are formed (the morphology's idiom); the eight
 *     neighbours are funnel shifts of three staged rows, the counts A, B, C, N1, N2 bit-sliced "exactly one / at least two"
 *     pairs over 64 pixels at once.  The context option "thin_route": 0 automatic, 1 stepwise (one launch per sub-iteration
 *     through a context workspace of two maps: the cross-check), 2 fused (one launch runs up to "thin_fuse" = 1..8 full
 *     iterations, 0 automatic, on a tile without leaving LDS, staged with 2 F halo rows: after j sub-iterations the staged
 *     region is exact except for a fringe of j pixels, which never reaches the tile).  Every setting gives the same bytes and
 *     the same info.  The deletions of every frame and iteration are summed on the device; a workgroup that arrives at a frame
 *     whose preceding iteration deleted nothing only copies its tile, and a tile stops when an iteration deleted nothing in
 *     its staged region.  max_iterations >= 1 queues every launch up front; max_iterations = 0 reads one device word between
 *     chunks of launches (8, 16, then 32 iterations) and stops when every frame has reported an iteration without deletions.
 * Not covered -- follow-ups: hit-or-miss; spur pruning of the skeleton; medial-axis radii (the skeleton with the distance
 * transform's value); thinning through the batch pipeline or the multi-GPU sharder; grey-level thinning. */
#define CANNY_HIP_THIN_MAX_ITERATIONS 16384
#define CANNY_HIP_THIN_INFO 4 /* long long per frame */
enum canny_hip_thin_method {
    CANNY_HIP_THIN_ZHANGSUEN = 0,
    CANNY_HIP_THIN_GUOHALL = 1
};
enum canny_hip_thin_part {
    CANNY_HIP_THIN_PART_PASSES = 0, /* all launches of a call that thin (with the bookkeeping between its chunks) */
    CANNY_HIP_THIN_PART_INFO = 1,   /* the zeroing and the final reduction to info */
    CANNY_HIP_THIN_PARTS = 2
};
/* d_bits, d_out_bits: n_frames * h * ((w + 7) / 8) bytes, any byte address; d_info: 4 * n_frames long long or NULL.  On the
 * context's stream.  max_iterations >= 1: fully asynchronous.  max_iterations = 0: THE CALL SYNCHRONISES THE STREAM BEFORE IT
 * RETURNS (it polls a device word between chunks of launches, as the hysteresis' host-driven route does). */
int canny_hip_dev_thin_bits(canny_hip_ctx *ctx, const unsigned char *d_bits, int n_frames, int h, int w, int method,
                            int max_iterations, unsigned char *d_out_bits, long long *d_info);
/* The same on the strong bit-plane that the preceding dev_canny of the same n_frames, h, w left in the context (another
 * geometry, or none yet: CANNY_HIP_ERR_INVALID; the plane is only read). */
int canny_hip_dev_canny_thin(canny_hip_ctx *ctx, int n_frames, int h, int w, int method, int max_iterations,
                             unsigned char *d_out_bits, long long *d_info);
/* Host buffers, synchronous: upload, the operator; only out_bits and, if not NULL, info come down. */
int canny_hip_thin_batch(canny_hip_ctx *ctx, const unsigned char *bits, int n_frames, int h, int w, int method,
                         int max_iterations, unsigned char *out_bits, long long *info);
/* Host-only, needs no device: the rule itself on host buffers. */
int canny_hip_thin_bits(const unsigned char *bits, int n_frames, int h, int w, int method, int max_iterations,
                        unsigned char *out_bits, long long *info);

/* ---- morphological reconstruction of packed bit maps ---------------------------------------------------------------------------
 * The connectivity-driven step that follows a threshold: keep the blobs that hold a seed (scipy.ndimage.binary_propagation,
 * imreconstruct, cv::floodFill from many seeds), fill the holes of blobs (scipy.ndimage.binary_fill_holes, imfill 'holes'),
 * drop the blobs that touch the frame border (skimage.segmentation.clear_border, imclearborder), and with two binarizations
 * hysteresis thresholding of any plane (skimage.filters.apply_hysteresis_threshold) -- on the packed layout of
 * canny_hip_dev_canny_bits, on the context's stream, without a download.  All three are ONE operator, reconstruction by
 * dilation: a start set is flooded inside a set that conducts, to its fixed point.  All bit operations; the fixed point is
 * unique: the same bytes on every run, route and machine.  tests/reconstruct_rule.py restates the rule in numpy,
 * csrc/canny_reconstruct_host.cpp as a stack flood in plain C++.
 * THE RULE:
 *   Bit maps [n_frames][h][(w + 7) / 8] bytes, rows MSB-first.  THE PAD BITS OF THE INPUTS ARE IGNORED (a column >= w is
 *     outside the frame), THE PAD BITS OF THE OUTPUT ARE WRITTEN 0, every output byte is written, EVERYTHING OUTSIDE THE
 *     FRAME IS NOT PART OF ANY SET, frames never see each other.
 *   M = the in-frame set of mask; B = the frame's border ring (row 0, row h-1, column 0, column w-1); c = connectivity, 4 or 8;
 *     R_c(S, G) = the pixels of G joined to a pixel of S & G by a c-connected path that lies inside G.
 *   CANNY_HIP_RECON_SEEDED = 0: out = R_c(marker, M) = scipy.ndimage.binary_propagation(marker & mask, structure_c, mask=mask).
 *   CANNY_HIP_RECON_FILL_HOLES = 1: out = frame \ R_c'(B, frame \ M) with c' = 12 - c: THE BACKGROUND TAKES THE DUAL
 *     CONNECTIVITY (foreground 8 <-> background 4) = scipy.ndimage.binary_fill_holes(mask, structure_c'); scipy's default is
 *     c = 8 here.  marker must be NULL.
 *   CANNY_HIP_RECON_CLEAR_BORDER = 2: out = M \ R_c(B, M).  marker must be NULL.
 *   info may be NULL; otherwise CANNY_HIP_RECON_INFO = 3 long long per frame, 8-byte aligned: [0] the set bits of the output,
 *     [1] the set bits of M, [2] the pixels of the start set: marker & M, resp. B \ M, resp. B & M.  Zeroed on the stream inside
 *     the call, fully written by it and not touched by a refused one.  It deliberately holds NO launch or sweep count: the
 *     bytes are the same on every run, route and machine, the number of launches that reach them is not.
 *   Facts (tests/test_reconstruct_rule.py): out is a subset of M for SEEDED and CLEAR_BORDER, M a subset of out for
 *     FILL_HOLES; all three are idempotent; SEEDED is monotone in the marker and returns M for marker = M; on the 96 x 160
 *     scene of the thinning (a ring 8 thick and a bar 7 thick, 1735 pixels) FILL_HOLES at c = 8 gives 3248 pixels (1513
 *     filled), SEEDED from the first set pixel keeps 427, CLEAR_BORDER keeps all 1735; the 7 x 7 diamond ring closed only by
 *     diagonal steps fills 13 pixels at c = 8 and 0 at c = 4.
 *   Limits: h, w in 1..32768, a plane < 2^31 pixels, at most 65535 frames; above: CANNY_HIP_ERR_UNSUPPORTED.  Bad enum values,
 *     a connectivity other than 4 or 8, NULL mandatory pointers, a marker where none is allowed, a misaligned info buffer, an
 *     output that overlaps marker, mask or info: CANNY_HIP_ERR_INVALID.  Both before anything is queued; nothing is written.
 *   Kernels (csrc/canny_reconstruct.hip): the flood's state lives IN THE CALLER'S OUTPUT where its rows are whole 8-byte
 *     aligned words, otherwise in a word-aligned copy in the context's thinning workspace.  An init kernel writes the start set,
 *     sweep launches grow it in place, a finish kernel turns it into the op's output.  The state only grows and never beyond
 *     the fixed point, so a workgroup that reads a neighbour's stale word is only delayed; words that another workgroup may
 *     write are accessed with relaxed atomics on aligned 64-bit words.  The context option "reconstruct_route": 0 automatic
 *     (the tile flood), 1 stepwise (a lane per word, one geodesic dilation step a launch through global memory: the
 *     cross-check, hopeless on long paths), 2 tile flood (a workgroup of 256 per tile of 8 x 64-bit words x 64 rows of a grid
 *     capped at 4096 floods the tile in LDS to its own fixed point behind a halo of one row and one word: per round
 *     s |= n & g, then the horizontal fill within the word in six doubling steps each way, csrc/canny_recon_words.h).  Both
 *     give the same bytes and the same info.  The waves that changed a word are counted per frame and launch on the device:
 *     a workgroup that arrives at a frame whose preceding launch changed nothing returns at once; launches are queued in
 *     chunks of 4, 8, 16, 32, then 64, and the host reads ONE word behind each chunk: the frames that still changed.
 *     THE CALLS THEREFORE SYNCHRONISE THE STREAM BEFORE THEY RETURN.  The read-only option "last_reconstruct_launches"
 *     answers the sweep launches the context's last call queued (0 on a fresh context): a diagnostic, run-dependent and not
 *     part of the result.
 *   Measured on an MI355X at 128 x 4K, c = 8: FILL_HOLES of Otsu-binarized frames 10.7 ms (28 launches),
 *     CLEAR_BORDER 12.4 ms, SEEDED on the strong plane 2.0 ms, on blobs 4.2 ms; the stepwise route 630, 590, 21.7 and 24.9 ms;
 *     canny_hip_dev_components_bits on the same masks 23.5, 5.7 and 54.9 ms.  A launch runs every tile once, so a path that
 *     winds through t tile borders takes up to t launches: a full-frame zigzag took 59,964 launches and 15 s, where the label
 *     pass takes 0.6 s -- ON SERPENTINE MAPS A LABEL PASS (canny_hip_dev_components_bits and a decision per label) IS FASTER.
 * Not covered -- follow-ups: grey-level reconstruction (h-maxima, imregionalmax); per-tile dirty stamps, so that a sweep visits
 * only tiles whose neighbourhood changed; a label-based route (run union-find, flag the roots that hold a seed) for serpentine
 * maps; an asynchronous form with a launch budget; reconstruction through the batch pipeline or the multi-GPU sharder. */
#define CANNY_HIP_RECON_INFO 3 /* long long per frame */
enum canny_hip_recon_op {
    CANNY_HIP_RECON_SEEDED = 0,
    CANNY_HIP_RECON_FILL_HOLES = 1,
    CANNY_HIP_RECON_CLEAR_BORDER = 2
};
enum canny_hip_recon_part {
    CANNY_HIP_RECON_PART_SWEEPS = 0, /* all sweep launches of a call (with the polls between its chunks) */
    CANNY_HIP_RECON_PART_INFO = 1,   /* the zeroing, the init and the finish kernels and the reduction to info */
    CANNY_HIP_RECON_PARTS = 2
};
/* d_marker (SEEDED; NULL otherwise), d_mask, d_out: n_frames * h * ((w + 7) / 8) bytes, any byte address; d_info:
 * 3 * n_frames long long or NULL.  On the context's stream; THE CALL SYNCHRONISES THE STREAM BEFORE IT RETURNS. */
int canny_hip_dev_reconstruct_bits(canny_hip_ctx *ctx, const unsigned char *d_marker, const unsigned char *d_mask, int n_frames,
                                   int h, int w, int op, int connectivity, unsigned char *d_out, long long *d_info);
/* The same with the strong bit-plane that the preceding dev_canny of the same n_frames, h, w left in the context as the mask
 * (another geometry, or none yet: CANNY_HIP_ERR_INVALID; the plane is only read). */
int canny_hip_dev_canny_reconstruct(canny_hip_ctx *ctx, const unsigned char *d_marker, int n_frames, int h, int w, int op,
                                    int connectivity, unsigned char *d_out, long long *d_info);
/* Host buffers, synchronous: upload, the operator; only out and, if not NULL, info come down. */
int canny_hip_reconstruct_batch(canny_hip_ctx *ctx, const unsigned char *marker, const unsigned char *mask, int n_frames, int h,
                                int w, int op, int connectivity, unsigned char *out, long long *info);
/* Host-only, needs no device: the rule itself on host buffers, a stack flood. */
int canny_hip_reconstruct_bits(const unsigned char *marker, const unsigned char *mask, int n_frames, int h, int w, int op,
                               int connectivity, unsigned char *out, long long *info);

/* ---- grey-level morphology and median filtering of u8 planes -------------------------------------------------------------------
 * What prepares a plane BEFORE it is thresholded: cv::erode / cv::dilate / cv::morphologyEx on a grey image
 * (scipy.ndimage.grey_erosion / grey_dilation, minimum_filter / maximum_filter) and cv::medianBlur
 * (scipy.ndimage.median_filter), on u8 planes as they lie on the device (frames, warped frames, fused backgrounds, the smoothed
 * plane dev_canny left in the context), on the context's stream, without a download.  A top hat or black hat flattens uneven
 * lighting in front of CANNY_HIP_BIN_OTSU, a median removes salt and pepper in front of canny; the binarization, corner,
 * descriptor, warp, fusion and canny calls take the output as it is.  All integers: the same bytes on every run, route and
 * machine.  tests/gray_morph_rule.py restates the rule in numpy, csrc/canny_gray_morph_host.cpp in plain C++.
 * THE RULE:
 *   Planes.  Input and output [n_frames][h][w] u8, any byte address.  Every output byte is written.  There is no in-place form:
 *     buffers that overlap give CANNY_HIP_ERR_INVALID.
 *   Element.  The binary morphology's: rows[kh] words, kw and kh odd in 1..31, bit i of rows[j] the offset (i - kw / 2,
 *     j - kh / 2), filled by canny_hip_morph_element for rect, cross and ellipse; flat (no weights); the same checks.
 *   Primitives, B the set of the element's offsets:
 *       ERODE : out(p) = min over b in B of in(p + b)
 *       DILATE: out(p) = max over b in B of in(p - b)   -- the element reflected, as the binary operator does
 *     These are scipy.ndimage.grey_erosion / grey_dilation with footprint = B.
 *   Border, border_mode with border_value:
 *       CANNY_HIP_GRAY_BORDER_NEUTRAL = 0: the outside reads 255 in an erosion step and 0 in a dilation step (OpenCV's default
 *         for morphology; scipy mode='constant' with cval 255 or 0)
 *       CANNY_HIP_GRAY_BORDER_REPLICATE = 1: coordinates are clamped to the frame (scipy mode='nearest')
 *       CANNY_HIP_GRAY_BORDER_CONSTANT = 2: the outside reads border_value, 0..255, in every step (scipy mode='constant')
 *     border_value is ignored by the other two modes.
 *   Ops, iterations in 1..16 as in the binary operator:
 *       CANNY_HIP_GRAY_ERODE = 0, _DILATE = 1: the primitive `iterations` times in sequence
 *       CANNY_HIP_GRAY_OPEN  = 2: `iterations` erosions, then `iterations` dilations;  _CLOSE = 3: the dual
 *       CANNY_HIP_GRAY_GRADIENT = 4: DILATE - ERODE;  _TOPHAT = 5: in - OPEN;  _BLACKHAT = 6: CLOSE - in.  THE THREE DIFFERENCES
 *         SATURATE AT 0 (cv::subtract on u8): under CONSTANT borders OPEN need not lie below the input.
 *       CANNY_HIP_GRAY_MEDIAN = 7: the element must be the full 3 x 3 or 5 x 5 rectangle; out(p) is the (k^2 - 1) / 2-th
 *         smallest (counted from 0) of the k^2 window values: cv::medianBlur, scipy.ndimage.median_filter(size=k).  The border
 *         is REPLICATE (cv::medianBlur's own) or CONSTANT; NEUTRAL: CANNY_HIP_ERR_INVALID.  iterations repeats the median.
 *   Facts (tests/test_gray_morph_rule.py).  THRESHOLD DECOMPOSITION: for every thr, binarizing the result at thr (v > thr) is
 *     the binary operator on the plane binarized at thr -- ERODE, DILATE, OPEN, CLOSE under NEUTRAL and under CONSTANT 0 or 255
 *     (binary NEUTRAL, ZERO, ONE); the median of a 0/1 plane is the majority.  TWO-VALUED PLANES: on a plane of only 0 and 255
 *     the grey operator is the binary operator, byte for byte.
 *   Limits: h, w in 1..32768, a plane < 2^31 pixels, at most 65535 frames; above: CANNY_HIP_ERR_UNSUPPORTED.  Bad enum values,
 *     bad ranges, NULL mandatory pointers, a bad element, buffers that overlap: CANNY_HIP_ERR_INVALID.  Both before anything is
 *     queued; nothing is written.
 *   Kernels (csrc/canny_gray_morph.hip): one launch per primitive step; a workgroup of 256 per tile of 128 columns x 32 rows
 *     and trip of a grid capped at 4096, a lane owning four adjacent pixels of four rows.  The tile and its halo are staged in
 *     LDS as words of four pixels with the border rule put in where they are formed; the arithmetic is packed 16-bit min / max
 *     on the even and the odd bytes of a word side by side.  The context option "gray_morph_route": 0 automatic, 1 general
 *     (per element row the set offsets of its runs; MEDIAN: a rank by counting, per pixel), 2 fast (full rectangles: the
 *     horizontal run of kw, then the vertical run of kh, both by doubling in LDS; MEDIAN: a min / max selection network of 19
 *     or 99 exchanges; any other element runs the general route).  All routes give the same bytes.  Sequential steps go
 *     through two planes in the binary morphology's context workspace (and, for GRADIENT, the output buffer; no call reads
 *     what another left there); the saturating difference belongs
 *     to the last step's kernel.
 * The one part is timed through canny_hip_profile_part_get("gray_morph", CANNY_HIP_GRAY_PART_STEPS); with "profile_stage_mask"
 * it goes by bit 30 like the other features' parts.
 * Not covered -- follow-ups: window medians above 5 x 5 by histogram; iteration fusing (several steps a launch); s16 planes;
 * grey-level reconstruction; non-flat elements; grey morphology through the batch pipeline or the multi-GPU sharder. */
enum canny_hip_gray_op {
    CANNY_HIP_GRAY_ERODE = 0,
    CANNY_HIP_GRAY_DILATE = 1,
    CANNY_HIP_GRAY_OPEN = 2,
    CANNY_HIP_GRAY_CLOSE = 3,
    CANNY_HIP_GRAY_GRADIENT = 4,
    CANNY_HIP_GRAY_TOPHAT = 5,
    CANNY_HIP_GRAY_BLACKHAT = 6,
    CANNY_HIP_GRAY_MEDIAN = 7
};
enum canny_hip_gray_border {
    CANNY_HIP_GRAY_BORDER_NEUTRAL = 0,
    CANNY_HIP_GRAY_BORDER_REPLICATE = 1,
    CANNY_HIP_GRAY_BORDER_CONSTANT = 2
};
enum canny_hip_gray_part {
    CANNY_HIP_GRAY_PART_STEPS = 0, /* all primitive steps of a call */
    CANNY_HIP_GRAY_PARTS = 1
};
/* d_plane: n_frames * h * w bytes, any byte address, or NULL: the smoothed plane that the preceding dev_canny of the same
 * n_frames, h, w left in the context (any canny_hip_dev_canny* call; another geometry, or none yet: CANNY_HIP_ERR_INVALID;
 * the plane is only read).  d_out: n_frames * h * w bytes, any byte address; rows: kh words of HOST memory, copied at call
 * time.  Asynchronous, on the context's stream. */
int canny_hip_dev_gray_morph(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int op,
                             const unsigned *rows, int kw, int kh, int border_mode, int border_value, int iterations,
                             unsigned char *d_out);
/* Host buffers, synchronous: upload, the operator; out comes down. */
int canny_hip_gray_morph_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int op,
                               const unsigned *rows, int kw, int kh, int border_mode, int border_value, int iterations,
                               unsigned char *out);
/* Host-only, needs no device: the same rule on host buffers. */
int canny_hip_gray_morph(const unsigned char *imgs, int n_frames, int h, int w, int op, const unsigned *rows, int kw, int kh,
                         int border_mode, int border_value, int iterations, unsigned char *out);

/* ---- image pyramids: pyrDown, pyrUp and whole pyramids of u8 planes ----------------------------------------------------------
 * What maps a u8 plane to a plane of half or twice the size, low-passed: cv::pyrDown / cv::pyrUp / cv::buildPyramid on CV_8U,
 * on planes as they lie on the device (frames, warped frames, fused backgrounds, the smoothed plane dev_canny left in the
 * context), on the context's stream, without a download.  Every level is one contiguous [n_frames][h_l][w_l] block, so the
 * canny, corner, descriptor, binarization, grey-morphology, warp and fusion calls take a level as it lies (d_out + off_l) --
 * edges, corners and matches at half and quarter resolution, coarse-to-fine search.  All integers: the same bytes on every run,
 * route and machine.  tests/pyramid_rule.py restates the rule in numpy, csrc/canny_pyramid_host.cpp in plain C++.
 * THE RULE:
 *   Fold.  fold(p, n) is reflect-101 (cv::BORDER_DEFAULT, scipy mode='mirror'): 0 if n == 1; otherwise, while p < 0 or
 *     p >= n: p = -p if p < 0, else p = 2 (n - 1) - p.  THE LOOP MATTERS for n = 2 and 3.
 *   pyrDown, taps k = (1, 4, 6, 4, 1).  Input [n][h][w] u8, output [n][oh][ow] with oh = (h + 1) / 2, ow = (w + 1) / 2:
 *       out(y, x) = (sum over j, i in 0..4 of k[j] k[i] in(fold(2 y + j - 2, h), fold(2 x + i - 2, w)) + 128) >> 8
 *     The sum is at most 255 * 256, a horizontal partial sum at most 4080: the rule runs on 16-bit halves WITHOUT A CARRY.
 *     This is cv::pyrDown on CV_8U; it equals scipy.ndimage.correlate1d(k, mode='mirror') on both axes, [::2, ::2],
 *     (t + 128) >> 8.
 *   pyrUp.  Input [n][h][w], output [n][oh][ow] with oh in {2 h - 1, 2 h} and ow in {2 w - 1, 2 w}, THE CALLER'S CHOICE, so
 *     that level l + 1 goes back up onto an odd-sized level l.  Per axis, with s[-1] := s[min(1, w - 1)] and s[w] := s[w - 1]:
 *       even output 2 x     : s[x - 1] + 6 s[x] + s[x + 1]
 *       odd  output 2 x + 1 : 4 (s[x] + s[x + 1])
 *     and out = (the sum of the products of the two axes' weights + 32) >> 6; the weights of every output sum to 64, the sum is
 *     at most 16320.  The values do not depend on whether the last row or column is cropped.  This is the zero-inserted grid
 *     of 2 h x 2 w filtered by k (x) k with mode='mirror' (scipy), and cv::pyrUp in the interior.
 *   Pyramid.  Level 0 is the input and is not copied; level l = 1..levels is the pyrDown of level l - 1.  levels in
 *     1..CANNY_HIP_PYR_MAX_LEVELS and levels <= ceil(log2(max(h, w))), so that no level repeats a 1 x 1 plane.  The output is
 *     ONE buffer: level l at byte offset off_l as contiguous [n][h_l][w_l], off_1 = 0, off_(l+1) = off_l + n h_l w_l rounded up
 *     to a multiple of 256.  canny_hip_pyramid_layout answers (h_l, w_l, off_l, bytes_l) per level and the total, the end of
 *     the last level.  THE PAD BYTES between levels are never written.
 *   Facts (tests/test_pyramid_rule.py).  A CONSTANT PLANE stays constant under both operators.  FLIPS: pyrDown commutes with a
 *     flip of an axis of odd length (of even length the decimation grid moves); pyrUp commutes with a flip of an axis whose
 *     output has 2 s - 1 samples.  pyrDown then pyrUp of a LINEAR RAMP reproduces the ramp away from the border.
 *   Limits: h, w (and oh, ow) in 1..32768, a plane < 2^31 pixels, at most 65535 frames; above: CANNY_HIP_ERR_UNSUPPORTED.  NULL
 *     mandatory pointers, bad sizes, bad oh / ow, bad levels, an input and an output that overlap: CANNY_HIP_ERR_INVALID.  Both
 *     before anything is queued; nothing is written.  Every pointer may have any byte address.
 *   Kernels (csrc/canny_pyramid.hip): one launch per level; a workgroup of 256 per tile of 128 columns x 32 rows of the OUTPUT
 *     and trip of a grid capped at 4096.  The context option "pyramid_route": 0 automatic, 1 direct (a lane per output pixel,
 *     25 taps from global memory, every index folded: the cross-check), 2 tiled (a lane loads one word of four source bytes
 *     and takes its neighbours' by cross-lane moves; the horizontal five taps with decimation give partial sums kept as the
 *     two 16-bit halves of LDS words; the vertical five taps run on the packed halves; a lane stores four pixels as one word
 *     where aligned; tiles inside the frame load without a test, border tiles fold).  All routes give the same bytes.  pyrUp
 *     has one route: a lane produces blocks of 4 x 2 outputs from 3 x 4 source pixels on packed halves.
 * The two parts are timed through canny_hip_profile_part_get("pyramid", CANNY_HIP_PYR_PART_*); with "profile_stage_mask" they
 * go by bit 30 like the other features' parts.
 * Not covered -- follow-ups: two levels in one launch; Laplacian pyramids (s16 planes); cv::resize with arbitrary factors;
 * multi-scale corners and descriptors as one call; pyramids through the batch pipeline or the multi-GPU sharder; colour
 * planes. */
#define CANNY_HIP_PYR_MAX_LEVELS 15
enum canny_hip_pyr_part {
    CANNY_HIP_PYR_PART_DOWN = 0, /* every pyrDown launch of a call */
    CANNY_HIP_PYR_PART_UP = 1,
    CANNY_HIP_PYR_PARTS = 2
};
/* Host-only, needs no device: info[4 l + 0..3] = (h, w, offset, bytes) of level l + 1, l = 0..levels - 1; *total_bytes: the
 * size of the pyramid's buffer.  Both pointers are mandatory. */
int canny_hip_pyramid_layout(int n_frames, int h, int w, int levels, long long *info, long long *total_bytes);
/* One level.  d_plane: n_frames * h * w bytes, any byte address, or NULL: the smoothed plane that the preceding dev_canny of
 * the same n_frames, h, w left in the context (any canny_hip_dev_canny* call, bytes or shorts; another geometry, or none yet:
 * CANNY_HIP_ERR_INVALID; the plane is only read).  d_out: n_frames * ((h + 1) / 2) * ((w + 1) / 2) bytes.  Asynchronous, on
 * the context's stream. */
int canny_hip_dev_pyr_down(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, unsigned char *d_out);
/* All levels into d_out (total_bytes of the layout), one launch per level; level l is read back from d_out to make level
 * l + 1.  d_plane as above. */
int canny_hip_dev_pyramid(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int levels,
                          unsigned char *d_out);
/* d_plane [n_frames][h][w] is mandatory; d_out: n_frames * oh * ow bytes. */
int canny_hip_dev_pyr_up(canny_hip_ctx *ctx, const unsigned char *d_plane, int n_frames, int h, int w, int oh, int ow,
                         unsigned char *d_out);
/* Host buffers, synchronous: upload, the levels; the levels come down into out (the layout; its pad bytes are not written). */
int canny_hip_pyramid_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int levels,
                            unsigned char *out);
int canny_hip_pyr_up_batch(canny_hip_ctx *ctx, const unsigned char *imgs, int n_frames, int h, int w, int oh, int ow,
                           unsigned char *out);
/* Host-only, need no device: the same rule on host buffers. */
int canny_hip_pyramid(const unsigned char *imgs, int n_frames, int h, int w, int levels, unsigned char *out);
int canny_hip_pyr_up(const unsigned char *imgs, int n_frames, int h, int w, int oh, int ow, unsigned char *out);

/* ---- per-stage HIP-event timing (events are recorded on the launch stream) ----------------- */
int canny_hip_profile_enable(canny_hip_ctx *ctx, int on);
int canny_hip_profile_reset(canny_hip_ctx *ctx);
/* Synchronises the stream, then returns accumulated device milliseconds and launch count. */
int canny_hip_profile_get(canny_hip_ctx *ctx, int stage, double *total_ms, long *launches);
/* The same for the Hough passes, which are not stages of the map: part 0 vote, 1 peaks, 2 select + sort. */
int canny_hip_hough_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the four parts of the component labelling (CANNY_HIP_CC_PART_*). */
int canny_hip_components_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the two parts of the distance transform (CANNY_HIP_EDT_PART_*). */
int canny_hip_edt_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the three parts of the Hough segments (CANNY_HIP_SEGMENT_PART_*). */
int canny_hip_hough_segments_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);

/* ... and for the four parts of the contour chains (CANNY_HIP_CONTOUR_PART_*). */
int canny_hip_contours_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the four parts of the Hough circles (CANNY_HIP_CIRCLE_PART_*). */
int canny_hip_hough_circles_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the three parts of the polygon approximation (CANNY_HIP_POLYGON_PART_*). */
int canny_hip_polygons_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the two parts of the sub-pixel edgels (CANNY_HIP_EDGEL_PART_*). */
int canny_hip_edgels_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the one part of the line fits (CANNY_HIP_LINE_FIT_PART_*). */
int canny_hip_line_fits_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the one part of the circle fits (CANNY_HIP_CIRCLE_FIT_PART_*). */
int canny_hip_circle_fits_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the four parts of the chamfer matching (CANNY_HIP_CHAMFER_PART_*). */
int canny_hip_chamfer_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the three parts of the contour shape measures (CANNY_HIP_SHAPE_PART_*). */
int canny_hip_shapes_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the two parts of the edge curves (CANNY_HIP_CURVE_PART_*). */
int canny_hip_curves_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the four parts of the corners (CANNY_HIP_CORNER_PART_*). */
int canny_hip_corners_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the four parts of the descriptors and their matching (CANNY_HIP_DESC_PART_*). */
int canny_hip_descriptors_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the three parts of the motion estimate (CANNY_HIP_MOTION_PART_*). */
int canny_hip_motion_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the two parts of the frame alignment (CANNY_HIP_WARP_PART_*). */
int canny_hip_warp_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the two parts of the temporal fusion (CANNY_HIP_FUSE_PART_*). */
int canny_hip_fuse_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* ... and for the one part of the binary morphology (CANNY_HIP_MORPH_PART_*; bit 30 of "profile_stage_mask" like the others). */
int canny_hip_morph_profile_get(canny_hip_ctx *ctx, int part, double *total_ms, long *launches);
/* Every group of parts by name, for this and later features: feature is "stages" (the canny stages of
 * canny_hip_profile_get), "hough", "components", "edt", "hough_segments", "contours", "hough_circles", "polygons", "edgels",
 * "line_fits", "circle_fits", "chamfer", "shapes", "curves", "corners", "descriptors", "motion", "warp", "fuse", "morph",
 * "binarize" (CANNY_HIP_BIN_PART_*), "thin" (CANNY_HIP_THIN_PART_*), "reconstruct" (CANNY_HIP_RECON_PART_*), "gray_morph"
 * (CANNY_HIP_GRAY_PART_*) or "pyramid" (CANNY_HIP_PYR_PART_*; the five have no named getter and follow bit 30 of
 * "profile_stage_mask" like the others); the answer is the named getter's.  An unknown name, a part the group does not have or a NULL: CANNY_HIP_ERR_INVALID, nothing is written. */
int canny_hip_profile_part_get(canny_hip_ctx *ctx, const char *feature, int part, double *total_ms, long *launches);

/* ---- self-test hooks used by the GPU test-suite -------------------------------------------- */
/* Runs the DEVICE magnitude / angle-bin functions over every (gx,gy) in [-lim,lim]^2 and writes
 * tables indexed [gy+lim][gx+lim] to host memory. */
int canny_hip_selftest_mag_angle(canny_hip_ctx *ctx, int lim, short *magnitudes, unsigned char *bins);
/* The same tables from the per-pixel arithmetic of each Sobel+NMS kernel form, run by the kernels' own device helpers.
 * The bin is what the kernel's neighbour select returns when the four neighbour maxima are the codes 0, 45, 90, 135.
 * A magnitude word whose upper 16 bits are not zero is reported as -1.  lim in [0, 1020]. */
enum canny_hip_pixel_form {
    CANNY_HIP_PIXEL_LDS_TILE = 0,    /* the LDS-tiled kernel (magnitude_d8 / angle_bin_d8) */
    CANNY_HIP_PIXEL_PACKED_I16 = 1,  /* the packed-i16 marching kernel */
    CANNY_HIP_PIXEL_F32 = 2,         /* the f32 marching kernel, plain magnitude store */
    CANNY_HIP_PIXEL_F32_FLOOR = 3    /* the f32 marching kernel, PLANES threshold floor at 0 */
};
int canny_hip_selftest_sobel_pixel(canny_hip_ctx *ctx, int form, int lim, short *magnitudes, unsigned char *bins);
/* Measurement aid (bench.py): a plain device copy of nbytes (a multiple of 16; both pointers 16-byte aligned), launched
 * `launches` times on the context's stream; *avg_ms receives the average device time of one launch (HIP events attached
 * to the dispatch).  It calibrates what a 1:1 read/write stream reaches on THIS device beside the Sobel+NMS pass, whose
 * roofline is quoted against the 8 TB/s spec (the reference has no counterpart: src/cuda.cu:83-101 only ever copies
 * host<->device).  Synchronous. */
int canny_hip_probe_copy(canny_hip_ctx *ctx, const void *d_src, void *d_dst, size_t nbytes, int launches,
                         double *avg_ms);

/* Compares the Gaussian kernels' reciprocal-based division a/divisor with the IEEE divide for EVERY
 * float a in [0, 256] (1.13e9 values) on the device; *mismatches receives the number of differences and
 * *largest_mismatching_dividend the largest a that differed (0 if none). */
int canny_hip_selftest_div(canny_hip_ctx *ctx, float divisor, unsigned long long *mismatches,
                           float *largest_mismatching_dividend);
/* Same comparison for the one-instruction form a/divisor ~ fma(a, c, a) that the interior Gaussian waves
 * use when the full-window weight is within an ulp of 1 (c = 0 when it is exactly 1). */
int canny_hip_selftest_div_fma(canny_hip_ctx *ctx, float divisor, float c, unsigned long long *mismatches,
                               float *largest_mismatching_dividend);
/* Entry `index` of the built-in (divisor, c) table the kernels use; CANNY_HIP_ERR_INVALID past the end. */
int canny_hip_selftest_div_fma_table(int index, float *divisor, float *c);
/* Host-only (needs no device): the expansion step of the batch pipelines' compact transfer -- a bit map (rows MSB-first,
 * padded to bytes: height * ((width + 7) / 8) bytes) becomes the reference's short plane (0 / 255), or with to_u8 != 0 a
 * byte plane, written by n_threads pool threads exactly as canny_hip_canny_batch does it. */
int canny_hip_selftest_expand_bits(const unsigned char *bits, int height, int width, int to_u8, void *out, int n_threads);
/* Host-only: the order in which the waves of a marching launch (Gaussian, Sobel+NMS) take the n_segs x n_strips cells
 * of a frame -- border cells first, see march_cell_of in csrc/canny_kernels.h.  Writes n_segs * n_strips (segment, strip)
 * pairs to out_pairs. */
int canny_hip_selftest_march_order(int n_segs, int n_strips, int *out_pairs);
/* Host-only: number of CPUs in a sysfs-style list ("0-3,8,10-11" -> 7; 0 if malformed) -- the parser behind the
 * sharder's NUMA binding. */
int canny_hip_selftest_cpulist_count(const char *text);
/* The histogram pass of the automatic rules alone, launched exactly as canny_hip_dev_canny_auto launches it, on a
 * caller-supplied device plane of n_frames contiguous height x width frames: bytes (plane_is_u8 != 0) or shorts, values in
 * [0,255].  kind CANNY_HIP_AUTO_MEDIAN counts the values, CANNY_HIP_AUTO_QUANTILE counts min(magnitude, 256) of the
 * plane's Sobel magnitudes.  d_hist (device, n_frames x 257 unsigned int) is zeroed first; everything runs on the
 * context's stream and nothing is read back. */
int canny_hip_selftest_histogram(canny_hip_ctx *ctx, const void *d_plane, int plane_is_u8, int kind, int height, int width,
                                 int n_frames, unsigned int *d_hist);
/* The select pass alone: the rule (parameters as canny_hip_dev_canny_auto) on each of n_frames device histograms of 257
 * unsigned int; d_pairs (device, 2 * n_frames ints) receives the clamped pairs.  Asynchronous like the above. */
int canny_hip_selftest_select(canny_hip_ctx *ctx, const unsigned int *d_hist, int n_frames, int rule, float low, float high,
                              int *d_pairs);
/* The device workspaces a context owns, one per index from 0 up, in the order of the members of the context (DESIGN.md
 * section 20 has a row for each): name (valid until the next call on the context), current device pointer (null while
 * it was never needed), allocated size, and what its words are to the kernels that read them:
 *   DATA:  bits, votes, histogram bins, flags, distances, pixels: a consumer only compares or adds these words;
 *   INDEX: words that some kernel uses as an index, offset or count that addresses memory (parent entries, CSR
 *          prefixes, stack slots, queue entries); a buffer with one such part is INDEX as a whole;
 *   CACHE: contents kept on purpose between calls (the Hough vote tables, with their key on the host).
 * After the members come the device staging of every cached batch pipeline ("pipe0.slot1.d_in" ...) and the workspaces
 * of the sub-contexts that pipelines 1.. compute on ("pipe1.plane_s" ...).  CANNY_HIP_ERR_INVALID past the end, and while
 * a canny_hip_dev_canny_stream batch is still pending (flush first).  Synchronises the context's stream, launches
 * nothing and changes nothing. */
enum canny_hip_workspace_kind { CANNY_HIP_WS_DATA = 0, CANNY_HIP_WS_INDEX = 1, CANNY_HIP_WS_CACHE = 2 };
int canny_hip_selftest_workspace(canny_hip_ctx *ctx, int index, const char **name, void **d_ptr, size_t *bytes, int *kind);
/* Host-only (needs no device, launches nothing, touches no context): how a launch whose grid is capped divides its work
 * (DESIGN.md section 21 has a row for each kind).  Such a kernel walks its work items in a grid-stride loop; the grid is
 * computed by a helper that takes sizes only, the launchers call that helper, and so does this entry.  out[0 .. 4] =
 * the work items of the launch (of ONE frame for the kinds whose grid has the frame as its second dimension), the items
 * a workgroup takes per trip of its loop, the workgroups, the trips = ceil(items / (workgroups * items per trip)), and
 * for CANNY_HIP_PLAN_EDT_ROWS the image rows a wave takes per item (1 or 8), 0 otherwise.
 *   sized by n_frames, height, width (valid as for every batch call; extra ignored except for HOUGH_VOTE_POINTS):
 *     POINTS_ROWS, CC_ROWS, CT_ROWS: image rows of the batch; CC_TILES: 64 x 64 tiles of the batch;
 *     EDT_ROWS: groups of out[4] rows; EDT_COLUMNS: 64-column strips of the batch;
 *     HOUGH_VOTE_STRONG / _BITS: 64-pixel words of a frame, one per lane and trip (the strong plane's count includes the
 *     rows that pad the last tile); HOUGH_VOTE_POINTS: the points of a frame's list, given in extra >= 0 (the grid is
 *     sized by pixels / 16, whatever the list holds); CIRCLES_VOTE_STRONG / _BITS: chunks of 64 words of a frame
 *   SCAN_FRAMES: n_frames alone (one workgroup, 256 frames per trip)
 *   sized by extra >= 1 alone: CC_FIXUP, PG_RECORDS: the record capacity; PG_SCAN_SUMS: the record capacity (items: its
 *     chunks of 2048 records); HOUGH_CELLS: numangle * numrho; CIRCLES_STEPS: gradient pairs; TO_GRAY: pixels (items:
 *     groups of 16)
 * CANNY_HIP_ERR_INVALID for an unknown kind, sizes a batch call would refuse, or extra < 1 where it counts. */
enum canny_hip_launch_plan_kind {
    CANNY_HIP_PLAN_POINTS_ROWS = 0,
    CANNY_HIP_PLAN_SCAN_FRAMES = 1,
    CANNY_HIP_PLAN_CC_TILES = 2,
    CANNY_HIP_PLAN_CC_ROWS = 3,
    CANNY_HIP_PLAN_CC_FIXUP = 4,
    CANNY_HIP_PLAN_CT_ROWS = 5,
    CANNY_HIP_PLAN_EDT_ROWS = 6,
    CANNY_HIP_PLAN_EDT_COLUMNS = 7,
    CANNY_HIP_PLAN_PG_RECORDS = 8,
    CANNY_HIP_PLAN_PG_SCAN_SUMS = 9,
    CANNY_HIP_PLAN_HOUGH_VOTE_STRONG = 10,
    CANNY_HIP_PLAN_HOUGH_VOTE_BITS = 11,
    CANNY_HIP_PLAN_HOUGH_VOTE_POINTS = 12,
    CANNY_HIP_PLAN_HOUGH_CELLS = 13,
    CANNY_HIP_PLAN_CIRCLES_VOTE_STRONG = 14,
    CANNY_HIP_PLAN_CIRCLES_VOTE_BITS = 15,
    CANNY_HIP_PLAN_CIRCLES_STEPS = 16,
    CANNY_HIP_PLAN_TO_GRAY = 17,
    CANNY_HIP_PLAN_KINDS = 18
};
int canny_hip_selftest_launch_plan(int kind, int n_frames, int height, int width, long long extra,
                                   unsigned long long *out);
/* Host-only, the same five outputs for the index-driven edgel kernel of canny_hip_dev_edgels_at (no kind of its own above:
 * the row kernel of canny_hip_dev_canny_edgels goes by CANNY_HIP_PLAN_POINTS_ROWS).  Its grid is (out[2], n_frames), sized
 * by the frame's pixels -- height * width / 1024 workgroups of 256 points, at least 1 and at most 1024 -- since only the
 * device knows the lists; n_points >= 1 is the list length of ONE frame, the items the loop walks. */
int canny_hip_selftest_edgels_plan(int n_frames, int height, int width, unsigned long long n_points,
                                   unsigned long long *out);
/* Host-only, the same five outputs for the capped launches of the chamfer matching (they have no kind above).  The batch is
 * walked in chunks of out[5] frames (see the section's Memory note); the plans are those of a full chunk:
 *   CANNY_HIP_CHAMFER_PLAN_COST:  the cost pass, items = the chunk's pixels, grid (out[2]);
 *   CANNY_HIP_CHAMFER_PLAN_CELLS: the direct score kernel and the candidate passes (histogram, collect), items = the
 *     n_templates * height * width anchors of ONE frame, grid (out[2], frames of the chunk).
 * The tiled score kernel's grid is (16 x 64 tiles of a frame, templates, frames of the chunk) and has no cap.
 * with_scores != 0: the caller passes d_scores (the cost plane, not the score workspace, limits the chunk). */
enum canny_hip_chamfer_plan { CANNY_HIP_CHAMFER_PLAN_COST = 0, CANNY_HIP_CHAMFER_PLAN_CELLS = 1 };
int canny_hip_selftest_chamfer_plan(int which, int n_frames, int height, int width, int n_templates, int with_scores,
                                    unsigned long long *out);
/* Host-only: how the tiled score kernel walks template t of the set these host arrays describe (validated as by
 * canny_hip_chamfer_set_create, which lays its set out with the same function): out[0] = bands of dy, out[1] = the
 * largest LDS tile of a band of t in u16 elements, out[2] = the largest of the whole set (the launch's LDS), out[3] = the
 * route the automatic choice takes for the set (1 direct, 2 tiled). */
int canny_hip_selftest_chamfer_bands(const int *offsets, const short *points, int n_templates, int t, int *out);
/* Host-only, the same five outputs for the capped launches of the contour shape measures (they have no kind above); both
 * are sized by the record capacity >= 1 alone:
 *   CANNY_HIP_SHAPES_PLAN_RECORDS:   the measure and the emit kernel, one wave per record and trip, 4 records per
 *     workgroup, at most 65536 workgroups;
 *   CANNY_HIP_SHAPES_PLAN_SCAN_SUMS: the scan's pass over its chunks of 2048 records (the polygons' scan, unchanged): one
 *     workgroup, 256 chunks per trip. */
enum canny_hip_shapes_plan { CANNY_HIP_SHAPES_PLAN_RECORDS = 0, CANNY_HIP_SHAPES_PLAN_SCAN_SUMS = 1 };
int canny_hip_selftest_shapes_plan(int which, unsigned long long capacity, unsigned long long *out);
/* Host-only, the same five outputs for the one capped launch shape of the edge curves (it has no kind above): the count
 * and the write kernel walk the image rows of the batch, one wave per row and trip, 4 rows per workgroup, at most 65536
 * workgroups.  Sized by n_frames, height, width, valid as for a curves call. */
int canny_hip_selftest_curves_plan(int n_frames, int height, int width, unsigned long long *out);
/* Host-only, the same five outputs for the capped launches of the corners (they have no kind above):
 *   CANNY_HIP_CORNERS_PLAN_TILES: the two passes over the plane (maximum; histograms and collect), items = the 64 x 16
 *     tiles of ONE frame, one per workgroup and trip, grid (out[2], frames of the chunk), at most 1024 workgroups in x;
 *     out[5] = frames of a chunk;
 *   CANNY_HIP_CORNERS_PLAN_ARITH: canny_hip_dev_corners_arith, items = n triples, 256 per workgroup, at most 1024
 *     workgroups (n_frames, height, width are not read).
 * out holds 6 words. */
enum canny_hip_corners_plan { CANNY_HIP_CORNERS_PLAN_TILES = 0, CANNY_HIP_CORNERS_PLAN_ARITH = 1 };
int canny_hip_selftest_corners_plan(int which, int n_frames, int height, int width, unsigned long long n,
                                    unsigned long long *out);
/* Host-only, the same five outputs for the capped launches of the descriptors and their matching (no kind above):
 *   CANNY_HIP_DESCRIPTORS_PLAN_DESCRIBE: items = the n * stride record slots (n frames, stride = corners_max), one wave
 *     per slot, 4 per workgroup and trip, at most 2048 workgroups;
 *   CANNY_HIP_DESCRIPTORS_PLAN_MATCH: the match and the reverse launch, items = n * ceil(stride / 256) (n pairs, stride
 *     that of the side held in registers: the query's for the match, the train's for the reverse), one per workgroup and
 *     trip, at most 2048 workgroups.
 * 1 <= stride <= CANNY_HIP_HOUGH_MAX_LINES, n >= 1 and within the calls' limits.  out holds 5 words. */
enum canny_hip_descriptors_plan { CANNY_HIP_DESCRIPTORS_PLAN_DESCRIBE = 0, CANNY_HIP_DESCRIPTORS_PLAN_MATCH = 1 };
int canny_hip_selftest_descriptors_plan(int which, unsigned long long n, int stride, unsigned long long *out);
/* Host-only, the same five outputs for the capped launches of the motion estimate (no kind above), n_pairs >= 1 and at most
 * CANNY_HIP_MATCH_MAX_PAIRS, 1 <= hypotheses <= CANNY_HIP_MOTION_MAX_HYPOTHESES:
 *   CANNY_HIP_MOTION_PLAN_GATHER, CANNY_HIP_MOTION_PLAN_REFIT: items = the n_pairs pairs, one per workgroup and trip, at most
 *     2048 workgroups;
 *   CANNY_HIP_MOTION_PLAN_SCORE: items = n_pairs * ceil(hypotheses / 256), one (pair, block of 256 hypotheses) per workgroup
 *     and trip, at most 2048 workgroups.
 * out holds 5 words. */
enum canny_hip_motion_plan { CANNY_HIP_MOTION_PLAN_GATHER = 0, CANNY_HIP_MOTION_PLAN_SCORE = 1, CANNY_HIP_MOTION_PLAN_REFIT = 2 };
int canny_hip_selftest_motion_plan(int which, unsigned long long n_pairs, int hypotheses, unsigned long long *out);
/* Host-only, the same five outputs for the capped launch of the warp (no kind above): items = the n_out * ceil(out_h / 16) *
 * ceil(out_w / 64) output tiles, one per workgroup of 256 and trip, at most 4096 workgroups.  Dimensions within the warp's
 * limits.  With xform != NULL (one record of 8 words, its source frame taken as present) also what the tiled route does with
 * tile (tile_x, tile_y) of a frame warped from a src_h x src_w source: box receives 5 ints: 1 if the tile's footprint is
 * staged in LDS, 0 if the tile gathers directly (the footprint exceeds CANNY_HIP_WARP_LDS_BYTES, is empty, or the record is
 * not usable), then the clipped footprint x0, y0, x1, y1 (inclusive; x1 < x0 or y1 < y0: empty). */
int canny_hip_selftest_warp_plan(int n_out, int out_h, int out_w, unsigned long long *out, const long long *xform, int src_h,
                                 int src_w, int interp, int tile_x, int tile_y, int *box);
/* Host-only, the same five outputs for the two capped launches of the temporal fusion (no kind above): which = a
 * canny_hip_fuse_part.  FUSE: items = n_groups * ceil(h / 16) * ceil(w / 64) output tiles with n_groups = (n_frames -
 * group_len) / group_step + 1; MASK: items = n_frames * ceil(h / 16) * ceil(w / 64) (group_len and group_step are not read);
 * one tile per workgroup of 256 and trip, at most 4096 workgroups.  The fifth word of FUSE is the route that automatic takes
 * for a MEDIAN of group_len frames (1 registers, 2 passes).  Arguments within the limits of the calls. */
int canny_hip_selftest_fuse_plan(int which, int n_frames, int h, int w, int group_len, int group_step,
                                 unsigned long long *out);
/* Host-only, the same five outputs for the capped launch of one primitive step of the binary morphology (no kind above): items
 * = n_frames * ceil(h / 64) * ceil(ceil(w / 64) / 8) tiles, one per workgroup of 256 and trip, at most 4096 workgroups.  The
 * fifth word is the route that automatic takes for a full rectangle of kw x kh (1 general, 2 separable).  Arguments within
 * the limits of the calls. */
int canny_hip_selftest_morph_plan(int n_frames, int h, int w, int kw, int kh, unsigned long long *out);
/* Host-only, TEN words for the binarization (no kind above): the same five outputs for the launch that writes the bits under
 * the route automatic takes -- FIXED, OTSU and route 1: items = n_frames * ceil(h * ceil(w / 8) / 256) chunks of 256 output
 * bytes, one per workgroup of 256 and trip; route 2: items = n_frames * strips * segments, four (one a wave) per workgroup and
 * trip; at most 4096 workgroups -- with the fifth word the route automatic takes for ADAPTIVE_MEAN (1 straightforward,
 * 2 marching; 0 for the other methods).  out[5]: the useful columns of a marching strip; out[6]: the rows of a segment for
 * this kh; out[7]: the trips of the launch of route 1 (and of FIXED and OTSU); out[8]: the trips of route 2; out[9]: the
 * staged columns of a strip for this kw (out[5] + the halo it has room for).  kw, kh are checked for ADAPTIVE_MEAN only;
 * arguments within the limits of the calls. */
int canny_hip_selftest_binarize_plan(int n_frames, int h, int w, int method, int kw, int kh, unsigned long long *out);
/* Host-only, the same five outputs for the capped launch of the thinning (no kind above; every launch of a call has this
 * plan): items = n_frames * ceil(h / 64) * ceil(ceil(w / 64) / 8) tiles, one per workgroup of 256 and trip, at most 4096
 * workgroups.  fuse: 0, or the "thin_fuse" to report (1..8).  The fifth word is the number of full iterations a launch runs:
 * fuse, or for fuse = 0 what automatic takes (0 if automatic is the stepwise route).  It refuses what the calls refuse. */
int canny_hip_selftest_thin_plan(int n_frames, int h, int w, int fuse, unsigned long long *out);
/* Host-only, the same five outputs for the sweep launches of the reconstruction (no kind above).  route 2, and 0 where
 * automatic takes the tile flood: items = n_frames * ceil(h / 64) * ceil(ceil(w / 64) / 8) tiles, one per workgroup of 256 and
 * trip; route 1: items = n_frames * h * ceil(w / 64) words, 256 per workgroup and trip (also the plan of the init and finish
 * kernels); at most 4096 workgroups.  The fifth word is the route automatic takes (1 or 2).  It refuses what the calls refuse. */
int canny_hip_selftest_reconstruct_plan(int n_frames, int h, int w, int route, unsigned long long *out);
/* Host-only, the same five outputs for the capped launch of one primitive step of the grey-level morphology (no kind above):
 * items = n_frames * ceil(h / 32) * ceil(w / 128) tiles, one per workgroup of 256 and trip, at most 4096 workgroups.  The fifth
 * word is the route that automatic takes for op with a full rectangle of kw x kh (1 general, 2 fast); it depends on op, kw and
 * kh alone.  kw, kh odd in 1..31 (MEDIAN: 3 x 3 or 5 x 5); it refuses what the calls refuse. */
int canny_hip_selftest_gray_morph_plan(int n_frames, int h, int w, int op, int kw, int kh, unsigned long long *out);
/* Host-only, the same five outputs for the capped launch of one pyrDown of planes [n_frames][h][w] (no kind above): items =
 * n_frames * ceil(oh / 32) * ceil(ow / 128) tiles of the OUTPUT (oh = (h + 1) / 2, ow = (w + 1) / 2), one per workgroup of 256
 * and trip, at most 4096 workgroups; a pyrUp INTO planes of oh x ow has the same plan.  The fifth word is the route automatic
 * takes (1 direct, 2 tiled); it depends on nothing.  It refuses what the calls refuse. */
int canny_hip_selftest_pyramid_plan(int n_frames, int h, int w, unsigned long long *out);
/* Runs the fuse kernels' own device helper for the rounded mean over every pair c = 1..255, s = 0..255 c, and writes the
 * bytes to host memory as a table [255][CANNY_HIP_FUSE_MEAN_ROW]: out[(c - 1) * 65026 + s]; unused cells are 0. */
int canny_hip_selftest_fuse_mean(canny_hip_ctx *ctx, unsigned char *out);

#ifdef __cplusplus
}
#endif
#endif /* CANNY_HIP_H */
