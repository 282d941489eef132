// main.cpp -- the reference's command line (StevenChang5/Canny_Edge src/main.cpp:18-142) without
// the webcam and the GUI:  ./Main sigma minVal maxVal [-c] [-s] [-i in.pgm|in.ppm|in.jpg] [-o dir] [-p] [-n WxH] [-b dir]
//        [-l rho,theta_degrees,threshold[,lines_max]] [-g min_length,max_gap[,exclusive]] [-m min_area] [-t] [-w min_length] [-d] [-e]
//        [-r min_radius,max_radius,threshold,support[,min_dist[,cell_shift]]] [-y epsilon[,ratio]] [-u]
//        [-q quality_q16,min_dist,corners_max[,block[,k_q8]]] [-j upright|steered]
//
// Kept from the reference: the three positionals may appear anywhere relative to the flags
// (src/main.cpp:29-46); exactly three are required, otherwise the usage text is printed and the
// program exits with status 0 (:48-56); maxVal must exceed minVal and both must lie in [0,255]
// (:63-76), again exiting 0 with the reference's messages; -s shows the steps, -c selects the GPU
// entry point (cuda_canny) instead of canny().  In this build both run on the MI355X.
// Replaced: VideoCapture(0) 640x480 (:78-115) -> a binary PGM or a baseline JPEG given with -i (the JPEG is read as
// cv::imread(..., IMREAD_GRAYSCALE) reads it, include/canny_frames.h), or a synthetic frame of the webcam's size
// (-n overrides the size); imshow -> PGM (or, with -p, PNG) files in the -o directory.  A binary PPM (P6, maxval 255,
// RGB) is a colour frame: it is converted on the GPU with canny_hip_to_gray and the OpenCV rule, in place of the
// reference's cvtColor(frame, gray_frame, COLOR_BGR2GRAY) (:114); -s also writes that plane as canny_step0_gray.pgm.
// Added: -l runs the Hough line transform of the frame's edge map on the GPU as well (canny_hip_canny_hough) and writes
// one "rho theta votes" row per detected line, strongest first, to canny_lines.txt in the -o directory (to stdout
// without -o).  Without -l nothing changes.
// Added: -g min_length,max_gap[,exclusive] (with -l) also writes the segments along those lines, one "x0 y0 x1 y1 line
// support" row each, to canny_segments.txt (canny_hip_canny_hough_segments).  -g without -l is a usage error (exit 2).
// Added: -m labels the 8-connected components of the frame's edge map on the GPU (canny_hip_canny_components), drops those
// with fewer than min_area pixels and writes one "label left top width height area" row per kept component to
// canny_components.txt and the filtered map to canny_kept.pgm (.png with -p) in the -o directory (rows to stdout without
// -o).  Without -m nothing changes.
// Added: -w min_length links the frame's edge map into curves on the GPU (canny_hip_canny_curves): every edge pixel once, in
// order along its curve, curves split at junctions; one "start end points flags x0 y0 x1 y1 ..." line per curve with at
// least min_length points goes to canny_curves.txt (start and end are pixel indices r * width + c; flags:
// canny_hip_curve_flag).  A malformed -w is a usage error (exit status 2).  Without -w nothing changes.
// Added: -t follows the outer border of every component of the frame's edge map with at least min_area pixels (-m, default
// 1) on the GPU (canny_hip_canny_contours) and writes one "label n x0 y0 x1 y1 ..." line per contour to canny_contours.txt
// in the -o directory (stdout without -o).
// Added: -y epsilon[,ratio] (with -t) also approximates every contour by a polygon on the GPU (canny_hip_canny_polygons; the
// chains stay on the device): the tolerance is epsilon pixels plus ratio times the contour's own length, as
// approxPolyDP(c, epsilon + ratio * arcLength(c, true), true).  One "frame record vertices length area2 convex x0 y0 x1 y1
// ..." line per contour goes to canny_polygons.txt in the -o directory (stdout without -o); record is the label of
// canny_contours.txt, length is in 1/256 pixel, area2 is twice the polygon's area.  -y without -t and a malformed -y are
// usage errors (exit 2).
// Added: -u (with -t) also measures every contour on the GPU (canny_hip_canny_shapes; the chains stay on the device): one
// "frame record points hull_vertices area2 hull_area2 rect_edge rect_along_min rect_along_max rect_across rect_len2 x0 y0 x1
// y1 ..." line per contour goes to canny_shapes.txt in the -o directory (stdout without -o), the trailing pairs being the
// vertices of the convex hull.  -u without -t is a usage error (exit 2).
// Added: -d runs the exact Euclidean distance transform of the frame's edge map on the GPU (canny_hip_canny_edt) and writes
// canny_dist.pgm (.png with -p) to the -o directory (the current one without -o): one byte per pixel,
// min(255, floor(sqrt(dist2))), 255 everywhere for a map without edge pixels.  Without -d nothing changes.
// Added: -r min_radius,max_radius,threshold,support[,min_dist[,cell_shift]] detects the circles of the frame's edge map on the
// GPU (canny_hip_canny_hough_circles) and writes one "frame x y radius votes support" row per circle, in candidate order,
// to canny_circles.txt in the -o directory (stdout without -o); x and y are the centre in pixels (multiples of 0.5).  A
// malformed -r is a usage error (exit 2).  Without -r nothing changes.
// Added: -f options (with -l and -g) also computes the sub-pixel line fit of every segment on the GPU
// (canny_hip_canny_hough_line_fits) and writes one "x0 y0 x1 y1 cx cy dx dy n rms maxd degenerate" row per segment to
// canny_line_fits.txt.  -f without -l and -g, or with anything but 0..3, is a usage error (exit 2).
// Added: -k band,trim_q8[,options] (with -r) also computes the sub-pixel circle fit of every circle on the GPU
// (canny_hip_canny_hough_circle_fits) and writes one "frame cx cy r n rms maxd sectors trim_failed degenerate" row per
// circle to canny_circle_fits.txt.  -k without -r, or with a band outside 0..4, a negative trim or options outside 0..3, is
// a usage error (exit 2).
// Added: -q quality_q16,min_dist,corners_max[,block[,k_q8]] finds the corners of the frame's smoothed plane on the GPU
// (canny_hip_canny_corners; Shi-Tomasi, or Harris when k_q8 is given) and writes one "frame x y response rank" line per
// corner to canny_corners.txt.  A malformed -q is a usage error (exit 2).  Without -q nothing changes.
// Added: -j upright|steered (with -q) also describes every corner on the GPU (canny_hip_canny_corner_descriptors; steered:
// the pattern turned to the patch's intensity centroid) and writes one "x y k border" and 64 hex digits (words 0..3, 16
// digits each) per corner to canny_descriptors.txt.  -j without -q, or with another word, is a usage error (exit 2).  (-b
// is the batch directory, so the descriptors took the next free letter.)
// Added: -x a.pgm[:b.pgm...],trunc_q4,max_mean_q4,min_dist matches the frame's edge map against the shapes of the PGM files
// (their non-zero pixels, anchored at the centre) on the GPU (canny_hip_canny_chamfer) and writes one "frame x y template
// score mean" row per match, in order, to canny_matches.txt in the -o directory (stdout without -o); mean is the mean
// cost in pixels to four decimals.  A malformed -x is a usage error (exit 2).  Without -x nothing changes.
// Added: -z op,kw[,kh[,shape[,iterations]]] applies a binary morphology operator to the finished edge map on the GPU
// (canny_hip_canny_morph, the neutral border): op erode, dilate, open, close, gradient, tophat or blackhat; kw and kh (default
// kw) odd, 1..31; shape rect (default), cross or ellipse; iterations 1..16 (default 1).  The map (0 / 255) goes to
// canny_morph.pgm in the -o directory.  A malformed -z is a usage error (exit 2).  Without -z nothing changes.
// Added: -a method[,thr_or_c[,kw[,kh[,invert]]]] binarizes the input frame itself on the GPU (canny_hip_binarize_batch): method
// fixed (thr_or_c the threshold, -1..255, default 127), otsu (the frame's own threshold, printed as "otsu threshold t"; the
// other fields are ignored) or mean (the adaptive mean: thr_or_c the offset c, -255..255, default 7; kw and kh (default kw) odd,
// 3..255, default 31); invert 0 (default) or 1.  The map (0 / 255) goes to canny_binary.pgm in the -o directory.  A malformed
// -a is a usage error (exit 2).  Without -a nothing changes.
// Added: -v method[,max_iterations] thins a bit map to a one-pixel skeleton on the GPU (canny_hip_dev_thin_bits): method guohall
// or zhangsuen, max_iterations 0..16384 (default 0: to the fixed point).  With -a it is the binarized frame, binarized on the
// device (canny_hip_dev_binarize) and thinned there with no download in between; without -a the finished edge map
// (canny_hip_dev_canny_bits).  The skeleton (0 / 255) goes to canny_thin.pgm in the -o directory and "thin iterations D deleted
// N" to stdout.  A malformed -v is a usage error (exit 2).  Without -v nothing changes.
// Added: -R op[,connectivity[,thr]] reconstructs a bit map on the GPU (canny_hip_dev_reconstruct_bits): op fill (the holes of
// the blobs filled), clear (the blobs that touch the frame border dropped) or seeded; connectivity 4 or 8 (default 8).  The map
// is chosen as -v chooses it: with -a the binarized frame, binarized on the device, without -a the finished edge map
// (canny_hip_dev_canny_bits).  seeded needs -a fixed,... and thr (-1..255): its marker is a second FIXED binarization of the
// same plane at thr with the polarity of -a, so that -a fixed,lo -R seeded,8,hi is hysteresis thresholding of the gray plane,
// all on the device.  The map (0 / 255) goes to canny_reconstruct.pgm in the -o directory and "reconstruct set N mask M start
// S" to stdout.  A malformed -R, or seeded without -a fixed, is a usage error (exit 2).  Without -R nothing changes.
// Added: -G op,kw[,kh[,shape[,iterations[,border]]]] applies a grey-level operator to the input frame itself on the GPU
// (canny_hip_dev_gray_morph): op is a word of -z or median; kw, kh, shape and iterations as in -z (median: 3 or 5, square,
// rect); border neutral (the default; not for median, whose default is replicate), replicate or a constant 0..255.  The plane
// goes to canny_gray.pgm in the -o directory; with -a also given, the binarization of THAT plane, binarized on the device with
// no download in between, goes to canny_gray_binary.pgm (canny_binary.pgm stays the binarization of the input frame).  A
// malformed -G is a usage error (exit 2).  Without -G nothing changes.
// Added: -P levels[,up] builds the pyramid of the input frame on the GPU (canny_hip_dev_pyramid: level l is cv::pyrDown of level
// l - 1) and writes its levels to canny_pyr1.pgm .. canny_pyr<levels>.pgm in the -o directory; with up, level 1 is also brought
// back to the frame's size (canny_hip_dev_pyr_up, cv::pyrUp) into canny_pyr_up.pgm.  levels is 1..15 and at most
// ceil(log2(max(height, width))); a malformed -P is a usage error (exit 2).  Without -P nothing changes.
// Added: -e computes the sub-pixel edgel of every pixel of the frame's edge map on the GPU (canny_hip_canny_edgels) and
// writes one "x y gx gy mag dir refined" row per edge pixel, in raster order, to canny_edgels.txt in the -o directory
// (stdout without -o): x and y in pixels to three decimals, mag in grey levels, dir 0..3 (step (1,0), (1,1), (0,1), (1,-1)),
// refined 0 / 1.  Without -e nothing changes.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "canny_frames.h"
#include "canny_hip.h"
#include "utils.h"
#include "cuda.h"

#define WIDTH 640
#define HEIGHT 480

using namespace std;

// Binary PGM (P5) -> gray bytes, or with `channels` = 3 binary PPM (P6) -> interleaved R,G,B bytes.
static bool read_pgm(const string &path, vector<unsigned char> &px, int &height, int &width, int channels = 1)
{
    ifstream f(path, ios::binary);
    if (!f) return false;
    string magic;
    f >> magic;
    if (magic != (channels == 3 ? "P6" : "P5")) return false;
    auto next_int = [&](int &v) {
        f >> ws;
        while (f.peek() == '#') {
            string line;
            getline(f, line);
            f >> ws;
        }
        return (bool)(f >> v);
    };
    int maxv = 0;
    if (!next_int(width) || !next_int(height) || !next_int(maxv)) return false;
    if (width < 1 || height < 1 || maxv < 1 || maxv > 255) return false;
    if (channels == 3 && maxv != 255) return false;
    if ((long long)width * height > 0x7fffffffLL) return false;
    f.get(); // single whitespace after maxval
    px.resize((size_t)width * height * channels);
    f.read((char *)px.data(), (streamsize)px.size());
    return (size_t)f.gcount() == px.size();
}

// A frame file: binary PGM, or a JPEG (told by its first two bytes, not by its name).
static bool read_frame(const string &path, vector<unsigned char> &px, int &height, int &width)
{
    ifstream f(path, ios::binary);
    if (!f) return false;
    unsigned char magic[2] = {0, 0};
    f.read((char *)magic, 2);
    if (f.gcount() == 2 && magic[0] == 0xFF && magic[1] == 0xD8) {
        f.seekg(0, ios::end);
        const streamoff len = f.tellg();
        if (len < 2) return false; // tellg() failed (-1: a pipe, a directory) or nothing behind the magic
        vector<unsigned char> file((size_t)len);
        f.seekg(0);
        f.read((char *)file.data(), (streamsize)file.size());
        int st = canny_frames_jpeg_info(file.data(), file.size(), &height, &width);
        if (!st) {
            px.resize((size_t)width * height);
            st = canny_frames_jpeg_decode_gray(file.data(), file.size(), px.data(), px.size(), &height, &width);
        }
        if (st) cout << "ERROR: " << path << ": " << canny_frames_last_error() << endl;
        return st == 0;
    }
    if (f.gcount() == 2 && magic[0] == 'P' && magic[1] == '6') { // colour: to gray on the GPU, OpenCV's rule
        f.close();
        vector<unsigned char> rgb;
        if (!read_pgm(path, rgb, height, width, 3)) return false;
        px.resize((size_t)width * height);
        canny_hip_ctx *ctx = nullptr;
        int st = canny_hip_ctx_create(&ctx, 0);
        if (!st) st = canny_hip_to_gray(ctx, rgb.data(), CANNY_HIP_RGB8, height, width, px.data());
        if (st) cout << "ERROR: " << path << ": " << (ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st)) << endl;
        if (ctx) canny_hip_ctx_destroy(ctx);
        return st == 0;
    }
    f.close();
    return read_pgm(path, px, height, width);
}

static bool is_ppm(const string &path)
{
    if (path.empty()) return false;
    ifstream f(path, ios::binary);
    char magic[2] = {0, 0};
    f.read(magic, 2);
    return f.gcount() == 2 && magic[0] == 'P' && magic[1] == '6';
}

static bool is_frame_file(const std::filesystem::path &p)
{
    string ext = p.extension().string();
    transform(ext.begin(), ext.end(), ext.begin(), [](unsigned char c) { return (char)tolower(c); });
    return ext == ".pgm" || ext == ".jpg" || ext == ".jpeg";
}

// Deterministic test card: gray background, filled rectangles, a little noise (xorshift).
static void synthetic_frame(vector<unsigned char> &px, int height, int width)
{
    px.assign((size_t)width * height, 30);
    unsigned s = 42u;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 17;
        s ^= s << 5;
        return s;
    };
    int rects = (int)(((long long)width * height) / 8000 + 4);
    for (int i = 0; i < rects; i++) {
        int w = 8 + (int)(rnd() % (unsigned)(width / 6 > 8 ? width / 6 - 7 : 1));
        int h = 8 + (int)(rnd() % (unsigned)(height / 6 > 8 ? height / 6 - 7 : 1));
        int x0 = (int)(rnd() % (unsigned)width), y0 = (int)(rnd() % (unsigned)height);
        unsigned char lv = (unsigned char)(rnd() & 255u);
        for (int y = y0; y < y0 + h && y < height; y++)
            for (int x = x0; x < x0 + w && x < width; x++) px[(size_t)y * width + x] = lv;
    }
    for (auto &p : px) {
        int v = (int)p + (int)(rnd() % 17u) - 8;
        p = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

static bool png_output = false; // -p: results as PNG instead of PGM

static bool write_frame(const string &path, const unsigned char *px, int height, int width)
{
    return canny_frames_write_gray(path.c_str(), px, height, width) == CANNY_FRAMES_OK;
}

// -b dir: every *.pgm / *.jpg / *.jpeg of the directory (sorted by name, all of one size) goes through the stream-overlapped
// batch entry point in one call; the 0/255 edge maps come back as bytes and are written as <name>_edges.pgm.
// The reference has no such mode (it loops over webcam frames, src/main.cpp:120-137); SURVEY.md 8(f) item 1.
static int run_batch(const string &dir, const string &outdir, float sigma, int minVal, int maxVal)
{
    namespace fs = std::filesystem;
    vector<fs::path> files;
    error_code ec;
    for (const auto &e : fs::directory_iterator(dir, ec))
        if (e.is_regular_file() && is_frame_file(e.path())) files.push_back(e.path());
    if (ec || files.empty()) {
        cout << "ERROR: no .pgm / .jpg frames in " << dir << endl;
        return -1;
    }
    sort(files.begin(), files.end());
    int height = 0, width = 0;
    vector<unsigned char> frames, one;
    for (size_t i = 0; i < files.size(); i++) {
        int h = 0, w = 0;
        if (!read_frame(files[i].string(), one, h, w) || (i > 0 && (h != height || w != width))) {
            cout << "ERROR: Failed to open " << files[i].string() << " (or its size differs from the first frame)" << endl;
            return -1;
        }
        height = h;
        width = w;
        frames.insert(frames.end(), one.begin(), one.end());
    }
    const size_t frame_px = (size_t)height * width;
    vector<unsigned char> edges(frames.size());
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    const auto t0 = chrono::steady_clock::now();
    if (!st)
        st = canny_hip_canny_batch_u8(ctx, frames.data(), (int)files.size(), sigma, minVal, maxVal, height, width,
                                      edges.data());
    const chrono::duration<double> dt = chrono::steady_clock::now() - t0;
    if (st) {
        fprintf(stderr, "ERROR: %s\n", ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    const fs::path out = outdir.empty() ? fs::path(dir) : fs::path(outdir);
    for (size_t i = 0; i < files.size(); i++) {
        const fs::path dst = out / (files[i].stem().string() + (png_output ? "_edges.png" : "_edges.pgm"));
        if (!write_frame(dst.string(), edges.data() + i * frame_px, height, width)) {
            cout << "ERROR: Failed to write " << dst.string() << endl;
            return -1;
        }
    }
    cout << "Execution time: " << dt.count() << " seconds (" << files.size() << " frames of " << width << "x" << height
         << ")\n";
    return 0;
}

// canny_lines.txt (stdout without -o): "%.9g %.9g %d" per line, strongest first -- the one writer behind -l and -l -g
static int write_lines(const vector<float> &lines, const vector<int> &votes, int n_lines, const string &outdir)
{
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_lines.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_lines.txt\n", outdir.c_str());
        return 1;
    }
    for (int k = 0; k < n_lines; k++) fprintf(f, "%.9g %.9g %d\n", lines[2 * k], lines[2 * k + 1], votes[k]);
    if (f != stdout) fclose(f);
    return 0;
}

// -l: the lines of the frame's edge map
static int run_hough(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                     double rho, double theta_deg, int threshold, int lines_max, const string &outdir)
{
    const float theta = (float)(theta_deg * M_PI / 180.0);
    vector<float> lines((size_t)2 * max(lines_max, 1));
    vector<int> votes((size_t)max(lines_max, 1));
    int count = 0;
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st)
        st = canny_hip_canny_hough(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, (float)rho, theta, threshold,
                                   lines_max, 0.0f, (float)M_PI, lines.data(), votes.data(), nullptr, &count);
    if (st) {
        fprintf(stderr, "ERROR: -l: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    return write_lines(lines, votes, min(count, lines_max), outdir);
}

// -l with -g: the lines as above and the segments along them, "x0 y0 x1 y1 line support" per segment; with -f
// (fit_options >= 0) also the line fit of every segment, "x0 y0 x1 y1 cx cy dx dy n rms maxd degenerate" per segment
static int run_segments(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                        double rho, double theta_deg, int threshold, int lines_max, int min_length, int max_gap,
                        int exclusive, int fit_options, const string &outdir)
{
    const float theta = (float)(theta_deg * M_PI / 180.0);
    vector<float> lines((size_t)2 * max(lines_max, 1));
    vector<int> votes((size_t)max(lines_max, 1));
    vector<int> segs, fits;
    int count = 0, seg_count = 0, cap = 4096;
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    for (int pass = 0; !st && pass < 2; pass++) { // a second time only if the first capacity was too small
        segs.resize((size_t)cap * CANNY_HIP_SEGMENT_INTS);
        if (fit_options >= 0) {
            fits.resize((size_t)cap * CANNY_HIP_LINE_FIT_INTS);
            st = canny_hip_canny_hough_line_fits(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, (float)rho,
                                                 theta, threshold, lines_max, 0.0f, (float)M_PI, min_length, max_gap,
                                                 exclusive, fit_options, lines.data(), votes.data(), nullptr, &count,
                                                 segs.data(), cap, &seg_count, fits.data());
        } else {
            st = canny_hip_canny_hough_segments(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, (float)rho,
                                                theta, threshold, lines_max, 0.0f, (float)M_PI, min_length, max_gap,
                                                exclusive, lines.data(), votes.data(), nullptr, &count, segs.data(), cap,
                                                &seg_count);
        }
        if (seg_count <= cap) break;
        cap = seg_count;
    }
    if (st) {
        fprintf(stderr, "ERROR: %s: %s\n", fit_options >= 0 ? "-f" : "-g",
                st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    if (write_lines(lines, votes, min(count, lines_max), outdir)) return 1;
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_segments.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_segments.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < seg_count; j++) {
        const int *r = segs.data() + (size_t)j * CANNY_HIP_SEGMENT_INTS;
        fprintf(f, "%d %d %d %d %d %d\n", r[0], r[1], r[2], r[3], r[4], r[5]);
    }
    if (f != stdout) fclose(f);
    if (fit_options < 0) return 0;
    f = outdir.empty() ? stdout : fopen((outdir + "/canny_line_fits.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_line_fits.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < seg_count; j++) {
        const int *r = fits.data() + (size_t)j * CANNY_HIP_LINE_FIT_INTS;
        const unsigned flags = (unsigned)r[9];
        const double sdd = (double)(unsigned)r[10] + 4294967296.0 * (double)(unsigned)r[11];
        fprintf(f, "%.4f %.4f %.4f %.4f %.4f %.4f %.6f %.6f %d %.4f %.4f %d\n", r[0] / 65536.0, r[1] / 65536.0,
                r[2] / 65536.0, r[3] / 65536.0, r[4] / 65536.0, r[5] / 65536.0, r[6] / 1073741824.0, r[7] / 1073741824.0,
                r[8], sqrt(sdd / (r[8] > 0 ? r[8] : 1)) / 256.0, (flags & CANNY_HIP_LINE_FIT_MAXD_MASK) / 256.0,
                (flags & CANNY_HIP_LINE_FIT_DEGENERATE) ? 1 : 0);
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -m: the kept components of the frame's edge map and the map without the dropped ones
static int run_components(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                          int min_area, const string &outdir)
{
    const size_t n = (size_t)height * width;
    vector<unsigned char> kept(n);
    vector<int> stats;
    unsigned long long offsets[2] = {0, 0};
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    // counts first, then exactly the records there are
    if (!st)
        st = canny_hip_canny_components(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr,
                                        nullptr, nullptr, 0, offsets);
    if (!st) {
        stats.resize((size_t)offsets[1] * CANNY_HIP_CC_STATS + 1);
        st = canny_hip_canny_components(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr,
                                        kept.data(), stats.data(), offsets[1], offsets);
    }
    if (st) {
        fprintf(stderr, "ERROR: -m: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_components.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_components.txt\n", outdir.c_str());
        return 1;
    }
    for (unsigned long long k = 0; k < offsets[1]; k++) {
        const int *r = stats.data() + k * CANNY_HIP_CC_STATS;
        fprintf(f, "%llu %d %d %d %d %d\n", k + 1, r[CANNY_HIP_CC_STAT_LEFT], r[CANNY_HIP_CC_STAT_TOP],
                r[CANNY_HIP_CC_STAT_WIDTH], r[CANNY_HIP_CC_STAT_HEIGHT], r[CANNY_HIP_CC_STAT_AREA]);
    }
    if (f != stdout) fclose(f);
    if (!outdir.empty()) {
        const string path = outdir + "/canny_kept" + (png_output ? ".png" : ".pgm");
        if (!write_frame(path, kept.data(), height, width)) {
            fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
            return 1;
        }
    }
    return 0;
}

// -t: the outer contour chain of every kept component, one "label n x0 y0 x1 y1 ..." line each
static int run_contours(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                        int min_area, const string &outdir)
{
    vector<unsigned long long> chain(1, 0);
    vector<int> points;
    unsigned long long offsets[2] = {0, 0}, point_offsets[2] = {0, 0};
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    // counts first, then exactly the chains there are
    if (!st)
        st = canny_hip_canny_contours(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr, 0,
                                      offsets, nullptr, nullptr, 0, point_offsets);
    if (!st) {
        chain.resize((size_t)offsets[1] + 1);
        points.resize((size_t)point_offsets[1] + 1);
        st = canny_hip_canny_contours(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr,
                                      offsets[1], offsets, chain.data(), points.data(), point_offsets[1], point_offsets);
    }
    if (st) {
        fprintf(stderr, "ERROR: -t: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_contours.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_contours.txt\n", outdir.c_str());
        return 1;
    }
    for (unsigned long long k = 0; k < offsets[1]; k++) {
        fprintf(f, "%llu %llu", k + 1, chain[k + 1] - chain[k]);
        for (unsigned long long q = chain[k]; q < chain[k + 1]; q++) fprintf(f, " %d %d", points[q] % width, points[q] / width);
        fprintf(f, "\n");
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -w: the edge curves of the frame's map with at least min_length points, one "start end points flags x0 y0 x1 y1 ..." line
// each: the record (start and end as pixel indices r * width + c), then the points
static int run_curves(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                      int min_length, const string &outdir)
{
    vector<unsigned long long> chain(1, 0);
    vector<int> points, records;
    unsigned long long offsets[2] = {0, 0}, point_offsets[2] = {0, 0};
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    // counts first, then exactly the curves there are
    if (!st)
        st = canny_hip_canny_curves(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_length, nullptr, 0,
                                    offsets, nullptr, nullptr, 0, point_offsets);
    if (!st) {
        chain.resize((size_t)offsets[1] + 1);
        records.resize((size_t)offsets[1] * CANNY_HIP_CURVE_RECORD + 1);
        points.resize((size_t)point_offsets[1] + 1);
        st = canny_hip_canny_curves(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_length, records.data(),
                                    offsets[1], offsets, chain.data(), points.data(), point_offsets[1], point_offsets);
    }
    if (st) {
        fprintf(stderr, "ERROR: -w: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_curves.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_curves.txt\n", outdir.c_str());
        return 1;
    }
    for (unsigned long long k = 0; k < offsets[1]; k++) {
        const int *rec = records.data() + k * CANNY_HIP_CURVE_RECORD;
        fprintf(f, "%d %d %d %d", rec[CANNY_HIP_CURVE_START], rec[CANNY_HIP_CURVE_END], rec[CANNY_HIP_CURVE_POINTS],
                rec[CANNY_HIP_CURVE_FLAGS]);
        for (unsigned long long q = chain[k]; q < chain[k + 1]; q++) fprintf(f, " %d %d", points[q] % width, points[q] / width);
        fprintf(f, "\n");
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -e: one sub-pixel edgel per edge pixel of the frame's map, in raster order: "x y gx gy mag dir refined" each.
static int run_edgels(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                      const string &outdir)
{
    vector<int> rec;
    unsigned long long offsets[2] = {0, 0};
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    // counts first, then exactly the records there are
    if (!st) st = canny_hip_canny_edgels(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, nullptr, 0, offsets, nullptr);
    if (!st && offsets[1]) {
        rec.resize((size_t)offsets[1] * CANNY_HIP_EDGEL_INTS);
        st = canny_hip_canny_edgels(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, rec.data(), offsets[1],
                                    offsets, nullptr);
    }
    if (st) {
        fprintf(stderr, "ERROR: -e: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_edgels.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_edgels.txt\n", outdir.c_str());
        return 1;
    }
    for (size_t k = 0; k < rec.size() / CANNY_HIP_EDGEL_INTS; k++) {
        const int *r = &rec[k * CANNY_HIP_EDGEL_INTS];
        const unsigned g = (unsigned)r[2], w3 = (unsigned)r[3];
        fprintf(f, "%.3f %.3f %d %d %.4f %u %u\n", r[0] / 256.0, r[1] / 256.0, (int)(short)(g & 0xffffu), (int)(short)(g >> 16),
                (w3 & CANNY_HIP_EDGEL_MAG_MASK) / 16.0, (w3 >> CANNY_HIP_EDGEL_DIR_SHIFT) & 3u,
                (w3 & CANNY_HIP_EDGEL_REFINED) ? 1u : 0u);
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -y (with -t): the polygon of every contour, "frame record vertices length area2 convex x0 y0 x1 y1 ..." each.  Only the
// polygons come down: the chains stay on the device.
static int run_polygons(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                        int min_area, unsigned epsilon_q8, unsigned ratio_q16, const string &outdir)
{
    vector<unsigned long long> vertex_offsets(1, 0);
    vector<int> vertices;
    vector<long long> measures;
    unsigned long long offsets[2] = {0, 0}, point_offsets[2] = {0, 0};
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    // counts first: a polygon has no more vertices than its chain has points
    if (!st)
        st = canny_hip_canny_contours(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr, 0,
                                      offsets, nullptr, nullptr, 0, point_offsets);
    if (!st) {
        vertex_offsets.resize((size_t)offsets[1] + 1);
        vertices.resize((size_t)point_offsets[1] + 1);
        measures.resize((size_t)offsets[1] * CANNY_HIP_POLYGON_MEASURES + 1);
        st = canny_hip_canny_polygons(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr,
                                      offsets[1], offsets, nullptr, nullptr, point_offsets[1], point_offsets, epsilon_q8,
                                      ratio_q16, vertex_offsets.data(), vertices.data(), point_offsets[1], measures.data());
    }
    if (st) {
        fprintf(stderr, "ERROR: -y: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_polygons.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_polygons.txt\n", outdir.c_str());
        return 1;
    }
    for (unsigned long long k = 0; k < offsets[1]; k++) {
        const long long *m = measures.data() + k * CANNY_HIP_POLYGON_MEASURES;
        fprintf(f, "0 %llu %lld %lld %lld %lld", k + 1, m[CANNY_HIP_POLYGON_VERTICES], m[CANNY_HIP_POLYGON_LENGTH_Q8],
                m[CANNY_HIP_POLYGON_AREA2], m[CANNY_HIP_POLYGON_CONVEX]);
        for (unsigned long long q = vertex_offsets[k]; q < vertex_offsets[k + 1]; q++)
            fprintf(f, " %d %d", vertices[q] % width, vertices[q] / width);
        fprintf(f, "\n");
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -u (with -t): the shape measures of every contour, "frame record points hull_vertices area2 hull_area2 rect_edge
// rect_along_min rect_along_max rect_across rect_len2 x0 y0 x1 y1 ..." each, the pairs being the hull.  Only the measures and
// the hulls come down: the chains stay on the device.
static int run_shapes(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                      int min_area, const string &outdir)
{
    vector<unsigned long long> hull_offsets(1, 0);
    vector<int> hull;
    vector<long long> measures;
    unsigned long long offsets[2] = {0, 0}, point_offsets[2] = {0, 0};
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    // counts first: a hull has no more vertices than its chain has points
    if (!st)
        st = canny_hip_canny_contours(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr, 0,
                                      offsets, nullptr, nullptr, 0, point_offsets);
    if (!st) {
        hull_offsets.resize((size_t)offsets[1] + 1);
        hull.resize((size_t)point_offsets[1] + 1);
        measures.resize((size_t)offsets[1] * CANNY_HIP_SHAPE_WORDS + 1);
        st = canny_hip_canny_shapes(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, min_area, nullptr, offsets[1],
                                    offsets, nullptr, nullptr, point_offsets[1], point_offsets, hull_offsets.data(),
                                    hull.data(), point_offsets[1], measures.data());
    }
    if (st) {
        fprintf(stderr, "ERROR: -u: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_shapes.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_shapes.txt\n", outdir.c_str());
        return 1;
    }
    for (unsigned long long k = 0; k < offsets[1]; k++) {
        const long long *m = measures.data() + k * CANNY_HIP_SHAPE_WORDS;
        fprintf(f, "0 %llu %lld %lld %lld %lld %lld %lld %lld %lld %lld", k + 1, m[CANNY_HIP_SHAPE_POINTS],
                m[CANNY_HIP_SHAPE_HULL_VERTICES], m[CANNY_HIP_SHAPE_AREA2], m[CANNY_HIP_SHAPE_HULL_AREA2],
                m[CANNY_HIP_SHAPE_RECT_EDGE], m[CANNY_HIP_SHAPE_RECT_ALONG_MIN], m[CANNY_HIP_SHAPE_RECT_ALONG_MAX],
                m[CANNY_HIP_SHAPE_RECT_ACROSS], m[CANNY_HIP_SHAPE_RECT_LEN2]);
        for (unsigned long long q = hull_offsets[k]; q < hull_offsets[k + 1]; q++)
            fprintf(f, " %d %d", hull[q] % width, hull[q] / width);
        fprintf(f, "\n");
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -d: the distance of every pixel to the nearest edge pixel, as a byte image
static int run_edt(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                   const string &outdir)
{
    const size_t n = (size_t)height * width;
    vector<int> dist2(n);
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_canny_edt(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, dist2.data(), nullptr, nullptr);
    if (st) {
        fprintf(stderr, "ERROR: -d: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    vector<unsigned char> out(n);
    for (size_t i = 0; i < n; i++) {
        int root = 0; // integer square root, capped: 255^2 <= dist2 gives 255
        while (root < 255 && (root + 1) * (root + 1) <= dist2[i]) root++;
        out[i] = (unsigned char)root;
    }
    const string path = (outdir.empty() ? string(".") : outdir) + "/canny_dist" + (png_output ? ".png" : ".pgm");
    if (!write_frame(path, out.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    return 0;
}

// -z: a morphology operator on the frame's edge map -> canny_morph.pgm.  m: op, kw, kh, shape, iterations
static int run_morph(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal, const int *m,
                     const string &outdir)
{
    const size_t rb = ((size_t)width + 7) / 8;
    vector<unsigned char> bits(rb * height);
    unsigned rows[CANNY_HIP_MORPH_MAX_EXTENT];
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_morph_element(m[3], m[1], m[2], rows);
    if (!st) st = canny_hip_ctx_create(&ctx, 0);
    if (!st)
        st = canny_hip_canny_morph(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, m[0], rows, m[1], m[2],
                                   CANNY_HIP_MORPH_BORDER_NEUTRAL, m[4], bits.data(), nullptr);
    if (st) {
        fprintf(stderr, "ERROR: -z: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    vector<unsigned char> out((size_t)height * width);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            out[(size_t)y * width + x] = (bits[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1 ? 255 : 0;
    const string path = (outdir.empty() ? string(".") : outdir) + "/canny_morph" + (png_output ? ".png" : ".pgm");
    if (!write_frame(path, out.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    return 0;
}

// -a: the frame binarized -> canny_binary.pgm.  a: method, thr_or_c, kw, kh, invert
static int run_binarize(const vector<unsigned char> &frame, int height, int width, const int *a, const string &outdir)
{
    const size_t rb = ((size_t)width + 7) / 8;
    vector<unsigned char> bits(rb * height);
    int thr = 0;
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_binarize_batch(ctx, frame.data(), 1, height, width, a[0], a[1], a[2], a[3], a[4], bits.data(), nullptr, &thr);
    if (st) {
        fprintf(stderr, "ERROR: -a: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    if (a[0] == CANNY_HIP_BIN_OTSU) printf("otsu threshold %d\n", thr);
    vector<unsigned char> out((size_t)height * width);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            out[(size_t)y * width + x] = (bits[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1 ? 255 : 0;
    const string path = (outdir.empty() ? string(".") : outdir) + "/canny_binary" + (png_output ? ".png" : ".pgm");
    if (!write_frame(path, out.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    return 0;
}

// -G: a grey-level operator on the frame -> canny_gray.pgm and, with bin (the -a arguments), the binarization of that plane ->
// canny_gray_binary.pgm.  g: op, kw, kh, shape, iterations, border_mode, border_value
static int run_gray_morph(const vector<unsigned char> &frame, int height, int width, const int *g, const int *bin, const string &outdir)
{
    const size_t rb = ((size_t)width + 7) / 8, px = (size_t)height * width;
    vector<unsigned char> plane(px), bits(rb * height);
    unsigned rows[CANNY_HIP_MORPH_MAX_EXTENT];
    int thr = 0;
    canny_hip_ctx *ctx = nullptr;
    void *d_img = nullptr, *d_out = nullptr, *d_bits = nullptr, *d_thr = nullptr;
    int st = canny_hip_morph_element(g[3], g[1], g[2], rows);
    if (!st) st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_malloc(ctx, &d_img, px);
    if (!st) st = canny_hip_malloc(ctx, &d_out, px);
    if (!st && bin) st = canny_hip_malloc(ctx, &d_bits, bits.size());
    if (!st && bin) st = canny_hip_malloc(ctx, &d_thr, sizeof(int));
    if (!st) st = canny_hip_memcpy_h2d(ctx, d_img, frame.data(), px);
    if (!st)
        st = canny_hip_dev_gray_morph(ctx, (const unsigned char *)d_img, 1, height, width, g[0], rows, g[1], g[2], g[5], g[6], g[4],
                                      (unsigned char *)d_out);
    if (!st && bin)
        st = canny_hip_dev_binarize(ctx, (const unsigned char *)d_out, 1, height, width, bin[0], bin[1], bin[2], bin[3], bin[4],
                                    (unsigned char *)d_bits, nullptr, (int *)d_thr);
    if (!st) st = canny_hip_memcpy_d2h(ctx, plane.data(), d_out, px);
    if (!st && bin) st = canny_hip_memcpy_d2h(ctx, bits.data(), d_bits, bits.size());
    if (!st && bin) st = canny_hip_memcpy_d2h(ctx, &thr, d_thr, sizeof(int));
    if (st) fprintf(stderr, "ERROR: -G: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
    if (ctx) {
        for (void *p : {d_img, d_out, d_bits, d_thr})
            if (p) canny_hip_free(ctx, p);
        canny_hip_ctx_destroy(ctx);
    }
    if (st) return 1;
    const string dir = outdir.empty() ? string(".") : outdir, ext = png_output ? ".png" : ".pgm";
    if (!write_frame(dir + "/canny_gray" + ext, plane.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", (dir + "/canny_gray" + ext).c_str());
        return 1;
    }
    if (!bin) return 0;
    if (bin[0] == CANNY_HIP_BIN_OTSU) printf("gray otsu threshold %d\n", thr);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            plane[(size_t)y * width + x] = (bits[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1 ? 255 : 0;
    if (!write_frame(dir + "/canny_gray_binary" + ext, plane.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", (dir + "/canny_gray_binary" + ext).c_str());
        return 1;
    }
    return 0;
}

// -P: the levels 1..levels of the frame's pyramid on the device -> canny_pyr1.pgm .. canny_pyr<levels>.pgm and, with up,
// level 1 brought back to the frame's size -> canny_pyr_up.pgm
static int run_pyramid(const vector<unsigned char> &frame, int height, int width, int levels, bool up, const string &outdir)
{
    long long info[4 * CANNY_HIP_PYR_MAX_LEVELS], total = 0;
    int st = canny_hip_pyramid_layout(1, height, width, levels, info, &total);
    if (st) {
        fprintf(stderr, "ERROR: -P: a frame of %d x %d has no level %d\n", width, height, levels);
        return 1;
    }
    const size_t px = (size_t)height * width;
    vector<unsigned char> pyr((size_t)total), back(up ? px : 0);
    canny_hip_ctx *ctx = nullptr;
    void *d_img = nullptr, *d_pyr = nullptr, *d_up = nullptr;
    st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_malloc(ctx, &d_img, px);
    if (!st) st = canny_hip_malloc(ctx, &d_pyr, pyr.size());
    if (!st && up) st = canny_hip_malloc(ctx, &d_up, px);
    if (!st) st = canny_hip_memcpy_h2d(ctx, d_img, frame.data(), px);
    if (!st) st = canny_hip_dev_pyramid(ctx, (const unsigned char *)d_img, 1, height, width, levels, (unsigned char *)d_pyr);
    if (!st && up)
        st = canny_hip_dev_pyr_up(ctx, (const unsigned char *)d_pyr, 1, (int)info[0], (int)info[1], height, width,
                                  (unsigned char *)d_up);
    for (int l = 0; l < levels && !st; l++) // level by level: the pads were never written
        st = canny_hip_memcpy_d2h(ctx, pyr.data() + info[4 * l + 2], (unsigned char *)d_pyr + info[4 * l + 2], (size_t)info[4 * l + 3]);
    if (!st && up) st = canny_hip_memcpy_d2h(ctx, back.data(), d_up, px);
    if (st) fprintf(stderr, "ERROR: -P: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
    if (ctx) {
        for (void *p : {d_img, d_pyr, d_up})
            if (p) canny_hip_free(ctx, p);
        canny_hip_ctx_destroy(ctx);
    }
    if (st) return 1;
    const string dir = outdir.empty() ? string(".") : outdir, ext = png_output ? ".png" : ".pgm";
    for (int l = 0; l < levels; l++) {
        const string path = dir + "/canny_pyr" + to_string(l + 1) + ext;
        if (!write_frame(path, pyr.data() + info[4 * l + 2], (int)info[4 * l], (int)info[4 * l + 1])) {
            fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
            return 1;
        }
    }
    if (up && !write_frame(dir + "/canny_pyr_up" + ext, back.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", (dir + "/canny_pyr_up" + ext).c_str());
        return 1;
    }
    return 0;
}

// -v: a bit map of the frame thinned on the device -> canny_thin.pgm.  bin: the -a arguments (method, thr_or_c, kw, kh, invert)
// or nullptr for the finished edge map; v: method, max_iterations
static int run_thin(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal, const int *bin,
                    const int *v, const string &outdir)
{
    const size_t rb = ((size_t)width + 7) / 8, px = (size_t)height * width;
    vector<unsigned char> bits(rb * height);
    long long info[CANNY_HIP_THIN_INFO] = {0, 0, 0, 0};
    canny_hip_ctx *ctx = nullptr;
    void *d_img = nullptr, *d_bits = nullptr, *d_out = nullptr, *d_info = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_malloc(ctx, &d_img, px);
    if (!st) st = canny_hip_malloc(ctx, &d_bits, bits.size());
    if (!st) st = canny_hip_malloc(ctx, &d_out, bits.size());
    if (!st) st = canny_hip_malloc(ctx, &d_info, sizeof(info));
    if (!st) st = canny_hip_memcpy_h2d(ctx, d_img, frame.data(), px);
    if (!st && bin)
        st = canny_hip_dev_binarize(ctx, (const unsigned char *)d_img, 1, height, width, bin[0], bin[1], bin[2], bin[3], bin[4],
                                    (unsigned char *)d_bits, nullptr, nullptr);
    if (!st && !bin)
        st = canny_hip_dev_canny_bits(ctx, (const unsigned char *)d_img, sigma, minVal, maxVal, height, width, 1, (unsigned char *)d_bits);
    if (!st)
        st = canny_hip_dev_thin_bits(ctx, (const unsigned char *)d_bits, 1, height, width, v[0], v[1], (unsigned char *)d_out,
                                     (long long *)d_info);
    if (!st) st = canny_hip_memcpy_d2h(ctx, bits.data(), d_out, bits.size());
    if (!st) st = canny_hip_memcpy_d2h(ctx, info, d_info, sizeof(info));
    if (st) fprintf(stderr, "ERROR: -v: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
    if (ctx) {
        for (void *p : {d_img, d_bits, d_out, d_info})
            if (p) canny_hip_free(ctx, p);
        canny_hip_ctx_destroy(ctx);
    }
    if (st) return 1;
    printf("thin iterations %lld deleted %lld\n", info[1], info[2]);
    vector<unsigned char> out(px);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            out[(size_t)y * width + x] = (bits[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1 ? 255 : 0;
    const string path = (outdir.empty() ? string(".") : outdir) + "/canny_thin" + (png_output ? ".png" : ".pgm");
    if (!write_frame(path, out.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    return 0;
}

// -R: a bit map of the frame reconstructed on the device -> canny_reconstruct.pgm.  bin: the -a arguments (method, thr_or_c, kw,
// kh, invert) or nullptr for the finished edge map; r: op, connectivity, thr of the marker (seeded)
static int run_reconstruct(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                           const int *bin, const int *r, const string &outdir)
{
    const size_t rb = ((size_t)width + 7) / 8, px = (size_t)height * width;
    vector<unsigned char> bits(rb * height);
    long long info[CANNY_HIP_RECON_INFO] = {0, 0, 0};
    canny_hip_ctx *ctx = nullptr;
    void *d_img = nullptr, *d_bits = nullptr, *d_marker = nullptr, *d_out = nullptr, *d_info = nullptr;
    const bool seeded = r[0] == CANNY_HIP_RECON_SEEDED;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_malloc(ctx, &d_img, px);
    if (!st) st = canny_hip_malloc(ctx, &d_bits, bits.size());
    if (!st) st = canny_hip_malloc(ctx, &d_marker, bits.size());
    if (!st) st = canny_hip_malloc(ctx, &d_out, bits.size());
    if (!st) st = canny_hip_malloc(ctx, &d_info, sizeof(info));
    if (!st) st = canny_hip_memcpy_h2d(ctx, d_img, frame.data(), px);
    if (!st && bin)
        st = canny_hip_dev_binarize(ctx, (const unsigned char *)d_img, 1, height, width, bin[0], bin[1], bin[2], bin[3], bin[4],
                                    (unsigned char *)d_bits, nullptr, nullptr);
    if (!st && !bin)
        st = canny_hip_dev_canny_bits(ctx, (const unsigned char *)d_img, sigma, minVal, maxVal, height, width, 1, (unsigned char *)d_bits);
    if (!st && seeded) // the marker: the same plane at the second threshold, the polarity of -a
        st = canny_hip_dev_binarize(ctx, (const unsigned char *)d_img, 1, height, width, CANNY_HIP_BIN_FIXED, r[2], 3, 3, bin[4],
                                    (unsigned char *)d_marker, nullptr, nullptr);
    if (!st)
        st = canny_hip_dev_reconstruct_bits(ctx, seeded ? (const unsigned char *)d_marker : nullptr, (const unsigned char *)d_bits, 1,
                                            height, width, r[0], r[1], (unsigned char *)d_out, (long long *)d_info);
    if (!st) st = canny_hip_memcpy_d2h(ctx, bits.data(), d_out, bits.size());
    if (!st) st = canny_hip_memcpy_d2h(ctx, info, d_info, sizeof(info));
    if (st) fprintf(stderr, "ERROR: -R: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
    if (ctx) {
        for (void *p : {d_img, d_bits, d_marker, d_out, d_info})
            if (p) canny_hip_free(ctx, p);
        canny_hip_ctx_destroy(ctx);
    }
    if (st) return 1;
    printf("reconstruct set %lld mask %lld start %lld\n", info[0], info[1], info[2]);
    vector<unsigned char> out(px);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            out[(size_t)y * width + x] = (bits[(size_t)y * rb + (x >> 3)] >> (7 - (x & 7))) & 1 ? 255 : 0;
    const string path = (outdir.empty() ? string(".") : outdir) + "/canny_reconstruct" + (png_output ? ".png" : ".pgm");
    if (!write_frame(path, out.data(), height, width)) {
        fprintf(stderr, "ERROR: cannot write %s\n", path.c_str());
        return 1;
    }
    return 0;
}

// -r: the circles of the frame's edge map, "frame x y radius votes support" per circle; with -k (fit != nullptr: band,
// trim_q8, options) also the circle fit of every circle, "frame cx cy r n rms maxd sectors trim_failed degenerate" per circle
static int run_circles(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                       const int *r, const int *fit, const string &outdir)
{
    const int centres_max = 256;
    vector<int> rec((size_t)centres_max * CANNY_HIP_CIRCLE_INTS), fits;
    int count = 0;
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st) {
        if (fit) {
            fits.resize((size_t)centres_max * CANNY_HIP_CIRCLE_FIT_INTS);
            st = canny_hip_canny_hough_circle_fits(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, r[0], r[1], r[5],
                                                   r[2], r[3], r[4], centres_max, fit[0], fit[1], fit[2], rec.data(), &count,
                                                   nullptr, fits.data());
        } else {
            st = canny_hip_canny_hough_circles(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, r[0], r[1], r[5],
                                               r[2], r[3], r[4], centres_max, rec.data(), &count, nullptr);
        }
    }
    if (st) {
        fprintf(stderr, "ERROR: %s: %s\n", fit ? "-k" : "-r",
                st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_circles.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_circles.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < count; j++) {
        const int *c = rec.data() + (size_t)j * CANNY_HIP_CIRCLE_INTS;
        fprintf(f, "0 %.1f %.1f %d %d %d\n", c[0] * 0.5, c[1] * 0.5, c[2], c[3], c[4]);
    }
    if (f != stdout) fclose(f);
    if (!fit) return 0;
    f = outdir.empty() ? stdout : fopen((outdir + "/canny_circle_fits.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_circle_fits.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < count; j++) {
        const int *c = fits.data() + (size_t)j * CANNY_HIP_CIRCLE_FIT_INTS;
        const unsigned flags = (unsigned)c[4];
        const double sdd = (double)(unsigned)c[6] + 4294967296.0 * (double)(unsigned)c[7];
        fprintf(f, "0 %.4f %.4f %.4f %d %.4f %.4f %04x %d %d\n", c[0] / 65536.0, c[1] / 65536.0, c[2] / 65536.0, c[3],
                sqrt(sdd / (c[3] > 0 ? c[3] : 1)) / 256.0, (flags & CANNY_HIP_CIRCLE_FIT_MAXD_MASK) / 256.0,
                (unsigned)c[5] & 0xffffu, (flags & CANNY_HIP_CIRCLE_FIT_TRIM_FAILED) ? 1 : 0,
                (flags & CANNY_HIP_CIRCLE_FIT_DEGENERATE) ? 1 : 0);
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -x: chamfer matching of the frame's edge map against the shapes of PGM files (their non-zero pixels, anchored at the
// centre), "frame x y template score mean" per match, in order; mean in pixels
static int run_chamfer(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                       const vector<string> &shapes, const int *a, const string &outdir)
{
    vector<int> offsets(1, 0);
    vector<short> points;
    for (const string &path : shapes) {
        vector<unsigned char> px;
        int h = 0, w = 0;
        if (!read_pgm(path, px, h, w)) {
            fprintf(stderr, "ERROR: -x: cannot read %s as a binary PGM\n", path.c_str());
            return 1;
        }
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (px[(size_t)y * w + x]) {
                    points.push_back((short)(x - w / 2));
                    points.push_back((short)(y - h / 2));
                }
        offsets.push_back((int)(points.size() / 2));
    }
    const int matches_max = 256;
    vector<int> rec((size_t)matches_max * CANNY_HIP_MATCH_INTS);
    int count = 0;
    canny_hip_ctx *ctx = nullptr;
    canny_hip_chamfer_set *set = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st) st = canny_hip_chamfer_set_create(ctx, offsets.data(), points.data(), (int)shapes.size(), &set);
    if (!st)
        st = canny_hip_canny_chamfer(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, set, a[0], a[1], a[2],
                                     matches_max, rec.data(), &count, nullptr);
    if (st) {
        fprintf(stderr, "ERROR: -x: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx); // the set dies with its context
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_matches.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_matches.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < count; j++) {
        const int *m = rec.data() + (size_t)j * CANNY_HIP_MATCH_INTS;
        fprintf(f, "0 %d %d %d %d %.4f\n", m[0], m[1], m[2], m[3], m[4] / 4096.0);
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -q: the corners of the frame's smoothed plane, "frame x y response rank" per corner, in order
static int run_corners(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                       const int *a, const string &outdir)
{
    const int corners_max = a[2], mode = a[4] >= 0 ? CANNY_HIP_CORNERS_HARRIS : CANNY_HIP_CORNERS_MIN_EIGEN;
    vector<long long> rec((size_t)corners_max * CANNY_HIP_CORNER_WORDS);
    int count = 0;
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st)
        st = canny_hip_canny_corners(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, mode, a[3],
                                     a[4] >= 0 ? a[4] : 0, a[0], 0, a[1], corners_max, rec.data(), &count, nullptr, nullptr);
    if (st) {
        fprintf(stderr, "ERROR: -q: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *f = outdir.empty() ? stdout : fopen((outdir + "/canny_corners.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot write %s/canny_corners.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < count; j++) {
        const long long *c = rec.data() + (size_t)j * CANNY_HIP_CORNER_WORDS;
        fprintf(f, "0 %lld %lld %lld %lld\n", c[0], c[1], c[2], c[3]);
    }
    if (f != stdout) fclose(f);
    return 0;
}

// -q with -j: the corners as run_corners writes them, and their descriptors, "x y k border hex" per corner, in order
static int run_descriptors(const vector<unsigned char> &frame, int height, int width, float sigma, int minVal, int maxVal,
                           const int *a, int desc_options, const string &outdir)
{
    const int corners_max = a[2], mode = a[4] >= 0 ? CANNY_HIP_CORNERS_HARRIS : CANNY_HIP_CORNERS_MIN_EIGEN;
    vector<long long> rec((size_t)corners_max * CANNY_HIP_CORNER_WORDS);
    vector<unsigned long long> desc((size_t)corners_max * CANNY_HIP_DESC_WORDS);
    vector<int> meta((size_t)corners_max);
    int count = 0;
    canny_hip_ctx *ctx = nullptr;
    int st = canny_hip_ctx_create(&ctx, 0);
    if (!st)
        st = canny_hip_canny_corner_descriptors(ctx, frame.data(), 1, sigma, minVal, maxVal, height, width, mode, a[3],
                                                a[4] >= 0 ? a[4] : 0, a[0], 0, a[1], corners_max, desc_options, rec.data(),
                                                &count, desc.data(), meta.data());
    if (st) {
        fprintf(stderr, "ERROR: -j: %s\n", st == CANNY_HIP_ERR_RUNTIME && ctx ? canny_hip_last_error(ctx) : canny_hip_status_string(st));
        if (ctx) canny_hip_ctx_destroy(ctx);
        return 1;
    }
    canny_hip_ctx_destroy(ctx);
    FILE *fc = outdir.empty() ? stdout : fopen((outdir + "/canny_corners.txt").c_str(), "w");
    FILE *fd = outdir.empty() ? stdout : fopen((outdir + "/canny_descriptors.txt").c_str(), "w");
    if (!fc || !fd) {
        fprintf(stderr, "ERROR: cannot write %s/canny_descriptors.txt\n", outdir.c_str());
        return 1;
    }
    for (int j = 0; j < count; j++) {
        const long long *c = rec.data() + (size_t)j * CANNY_HIP_CORNER_WORDS;
        fprintf(fc, "0 %lld %lld %lld %lld\n", c[0], c[1], c[2], c[3]);
    }
    for (int j = 0; j < count; j++) {
        const long long *c = rec.data() + (size_t)j * CANNY_HIP_CORNER_WORDS;
        const unsigned long long *d = desc.data() + (size_t)j * CANNY_HIP_DESC_WORDS;
        fprintf(fd, "%lld %lld %d %d %016llx%016llx%016llx%016llx\n", c[0], c[1], meta[j] & 255, meta[j] >> 8, d[0], d[1], d[2],
                d[3]);
    }
    if (fc != stdout) fclose(fc);
    if (fd != stdout) fclose(fd);
    return 0;
}

int main(int argc, char *argv[])
{
    // The batch pipeline wants its upload, compute and download streams on separate hardware queues; HIP reads this
    // when its runtime initialises (first HIP call, below), and the library leaves the environment alone.
    setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0);
    float sigma;
    int minVal;
    int maxVal;
    bool use_gpu_entry = false;
    bool show_steps = false;
    string input, outdir, batch_dir;
    bool want_lines = false;
    double line_rho = 1.0, line_theta_deg = 1.0;
    int line_threshold = 0, lines_max = 256;
    bool want_segments = false;
    int seg_min_length = 0, seg_max_gap = 0, seg_exclusive = 0;
    bool want_components = false;
    int min_area = 1;
    bool want_dist = false;
    bool want_contours = false;
    bool want_curves = false;
    int curve_min_length = 1;
    bool want_circles = false;
    bool want_polygons = false;
    bool want_shapes = false;
    bool want_edgels = false;
    int fit_options = -1; // -f: the line fits of the segments; -1 = not asked for
    unsigned polygon_epsilon_q8 = 0, polygon_ratio_q16 = 0;
    int circle_args[6] = {0, 0, 0, 0, 0, 0}; // min_radius, max_radius, threshold, support, min_dist, cell_shift
    bool want_circle_fits = false;
    int circle_fit_args[3] = {0, 0, 0}; // -k: band, trim_q8, options
    vector<string> chamfer_shapes;      // -x: the PGM files of the shapes
    int chamfer_args[3] = {0, 0, 0};    // ... trunc_q4, max_mean_q4, min_dist
    bool want_corners = false;
    int corner_args[5] = {0, 0, 0, 3, -1}; // -q: quality_q16, min_dist, corners_max, block, k_q8 (-1: Shi-Tomasi)
    int desc_options = -1;                 // -j: -1 absent, 0 upright, CANNY_HIP_DESC_STEERED
    bool want_morph = false;
    int morph_args[5] = {0, 3, 3, 0, 1};   // -z: op, kw, kh, shape, iterations
    bool want_gray = false;
    bool want_pyramid = false, pyramid_up = false; // -P levels[,up]
    int pyramid_levels = 0;
    int gray_args[7] = {0, 3, 3, 0, 1, 0, 0}; // -G: op, kw, kh, shape, iterations, border_mode, border_value
    bool want_binarize = false;
    int bin_args[5] = {0, 127, 31, 31, 0}; // -a: method, thr_or_c, kw, kh, invert
    bool want_thin = false;
    int thin_args[2] = {CANNY_HIP_THIN_GUOHALL, 0}; // -v: method, max_iterations
    bool want_recon = false, recon_thr_given = false;
    int recon_args[3] = {CANNY_HIP_RECON_FILL_HOLES, 8, 0}; // -R: op, connectivity, thr of the marker (seeded)
    int width = WIDTH, height = HEIGHT;
    vector<string> values;

    for (int i = 1; i < argc; i++) {
        string arg = argv[i];
        if (arg == "-c") {
            use_gpu_entry = true;
        } else if (arg == "-s") {
            show_steps = true;
        } else if (arg == "-p") {
            png_output = true;
        } else if (arg == "-i" && i + 1 < argc) {
            input = argv[++i];
        } else if (arg == "-o" && i + 1 < argc) {
            outdir = argv[++i];
        } else if (arg == "-b" && i + 1 < argc) {
            batch_dir = argv[++i];
        } else if (arg == "-l" && i + 1 < argc) {
            const int got = sscanf(argv[++i], "%lf,%lf,%d,%d", &line_rho, &line_theta_deg, &line_threshold, &lines_max);
            if (got < 3) {
                fprintf(stderr, "ERROR: -l expects rho,theta_degrees,threshold[,lines_max]\n");
                exit(0);
            }
            want_lines = true;
        } else if (arg == "-g" && i + 1 < argc) {
            if (sscanf(argv[++i], "%d,%d,%d", &seg_min_length, &seg_max_gap, &seg_exclusive) < 2) {
                fprintf(stderr, "ERROR: -g expects min_length,max_gap[,exclusive]\n");
                exit(2);
            }
            want_segments = true;
        } else if (arg == "-f" && i + 1 < argc) {
            char *end = nullptr;
            const char *p = argv[++i];
            const long v = strtol(p, &end, 10);
            if (end == p || *end != '\0' || isspace((unsigned char)*p) || v < 0 || v > 3) {
                fprintf(stderr, "ERROR: -f expects options: 0, 1 (gate), 2 (refined only) or 3\n");
                exit(2);
            }
            fit_options = (int)v;
        } else if (arg == "-m" && i + 1 < argc) {
            if (sscanf(argv[++i], "%d", &min_area) != 1) {
                fprintf(stderr, "ERROR: -m expects min_area\n");
                exit(0);
            }
            want_components = true;
        } else if (arg == "-r" && i + 1 < argc) {
            int *c = circle_args;
            int got = 0; // whole comma-separated integers only: nothing empty, nothing behind the last one
            bool clean = true;
            for (const char *p = argv[++i]; clean; got++) {
                char *end = nullptr;
                const long v = strtol(p, &end, 10);
                clean = end != p && got < 6 && v >= -0x7fffffffL && v <= 0x7fffffffL;
                if (clean) c[got] = (int)v;
                if (!clean || *end == '\0') break;
                clean = *end == ',';
                p = end + 1;
            }
            got = clean ? got + 1 : 0;
            if (got < 4 || got > 6 || c[0] < 1 || c[1] < c[0] || c[4] < 0 || c[5] < 0 || c[5] > 3) {
                fprintf(stderr, "ERROR: -r expects min_radius,max_radius,threshold,support[,min_dist[,cell_shift]]\n");
                exit(2);
            }
            want_circles = true;
        } else if (arg == "-k" && i + 1 < argc) {
            int *c = circle_fit_args;
            int got = 0; // whole comma-separated integers only, as -r
            bool clean = true;
            for (const char *p = argv[++i]; clean; got++) {
                char *end = nullptr;
                const long v = strtol(p, &end, 10);
                clean = end != p && got < 3 && !isspace((unsigned char)*p) && v >= -0x7fffffffL && v <= 0x7fffffffL;
                if (clean) c[got] = (int)v;
                if (!clean || *end == '\0') break;
                clean = *end == ',';
                p = end + 1;
            }
            got = clean ? got + 1 : 0;
            if (got < 2 || got > 3 || c[0] < 0 || c[0] > CANNY_HIP_CIRCLE_FIT_MAX_BAND || c[1] < 0 || c[2] < 0 || c[2] > 3) {
                fprintf(stderr, "ERROR: -k expects band,trim_q8[,options]: band 0..4, trim_q8 >= 0 (1/256 px, 0 = off), options 0..3\n");
                exit(2);
            }
            want_circle_fits = true;
        } else if (arg == "-x" && i + 1 < argc) {
            // a.pgm[:b.pgm...],trunc_q4,max_mean_q4,min_dist: the last three commas separate whole integers
            const string spec = argv[++i];
            size_t cut[3];
            size_t at = string::npos;
            bool clean = true;
            for (int k = 2; k >= 0 && clean; k--) {
                at = spec.rfind(',', at == string::npos ? at : at - 1);
                clean = at != string::npos && at > 0;
                cut[k] = at;
            }
            for (int k = 0; k < 3 && clean; k++) {
                const string v = spec.substr(cut[k] + 1, (k < 2 ? cut[k + 1] : spec.size()) - cut[k] - 1);
                char *end = nullptr;
                const long n = strtol(v.c_str(), &end, 10);
                clean = !v.empty() && *end == '\0' && !isspace((unsigned char)v[0]) && n >= 0 && n <= 0x7fffffffL;
                chamfer_args[k] = (int)n;
            }
            chamfer_shapes.clear();
            for (size_t b = 0; clean && b <= cut[0];) {
                size_t e = spec.find(':', b);
                if (e == string::npos || e > cut[0]) e = cut[0];
                clean = e > b;
                chamfer_shapes.push_back(spec.substr(b, e - b));
                b = e + 1;
            }
            if (!clean || chamfer_shapes.empty() || chamfer_args[0] < 1 || chamfer_args[0] > CANNY_HIP_CHAMFER_MAX_TRUNC ||
                chamfer_args[1] >= chamfer_args[0]) {
                fprintf(stderr, "ERROR: -x expects a.pgm[:b.pgm...],trunc_q4,max_mean_q4,min_dist: 1/16 px, 1 <= trunc_q4 <= 4095, max_mean_q4 < trunc_q4\n");
                exit(2);
            }
        } else if (arg == "-y" && i + 1 < argc) {
            // one or two non-negative numbers, nothing empty, nothing behind the last one
            double v[2] = {0.0, 0.0};
            int got = 0;
            bool clean = true;
            for (const char *p = argv[++i]; clean; got++) {
                char *end = nullptr;
                const double d = strtod(p, &end);
                clean = end != p && got < 2 && std::isfinite(d) && d >= 0.0 && !isspace((unsigned char)*p);
                if (clean) v[got] = d;
                if (!clean || *end == '\0') break;
                clean = *end == ',';
                p = end + 1;
            }
            const double eq = std::floor(v[0] * 256.0 + 0.5), rq = std::floor(v[1] * 65536.0 + 0.5);
            if (!clean || eq > 4294967295.0 || rq >= 65536.0) {
                fprintf(stderr, "ERROR: -y expects epsilon[,ratio]: pixels >= 0 and a fraction of the contour's length in [0, 1)\n");
                exit(2);
            }
            polygon_epsilon_q8 = (unsigned)eq, polygon_ratio_q16 = (unsigned)rq;
            want_polygons = true;
        } else if (arg == "-u") {
            want_shapes = true;
        } else if (arg == "-d") {
            want_dist = true;
        } else if (arg == "-t") {
            want_contours = true;
        } else if (arg == "-q" && i + 1 < argc) {
            // three to five whole non-negative integers, nothing empty, nothing behind the last one
            int got = 0;
            bool clean = true;
            corner_args[3] = 3, corner_args[4] = -1;
            for (const char *p = argv[++i]; clean; got++) {
                char *end = nullptr;
                const long v = strtol(p, &end, 10);
                clean = end != p && got < 5 && v >= 0 && v <= 65536 && isdigit((unsigned char)*p);
                if (clean) corner_args[got] = (int)v;
                if (!clean || *end == '\0') break;
                clean = *end == ',';
                p = end + 1;
            }
            got++;
            const int b = corner_args[3];
            if (!clean || got < 3 || corner_args[2] < 1 || corner_args[2] > CANNY_HIP_HOUGH_MAX_LINES ||
                (b != 3 && b != 5 && b != 7) || corner_args[4] > CANNY_HIP_CORNERS_MAX_K_Q8) {
                fprintf(stderr, "ERROR: -q expects quality_q16,min_dist,corners_max[,block[,k_q8]]: quality in 1/65536 of the largest "
                                "response, 1 <= corners_max <= 4096, block 3, 5 or 7, k_q8 <= 64 (in 1/256) chooses Harris\n");
                exit(2);
            }
            want_corners = true;
        } else if (arg == "-j") {
            const string word = i + 1 < argc ? argv[++i] : "";
            if (word != "upright" && word != "steered") {
                fprintf(stderr, "ERROR: -j expects upright or steered (the descriptors of the corners of -q)\n");
                exit(2);
            }
            desc_options = word == "steered" ? CANNY_HIP_DESC_STEERED : 0;
        } else if (arg == "-z") {
            // op,kw[,kh[,shape[,iterations]]]: words and whole integers, nothing empty, nothing behind the last one
            static const char *const ops[] = {"erode", "dilate", "open", "close", "gradient", "tophat", "blackhat"};
            static const char *const shapes[] = {"rect", "cross", "ellipse"};
            vector<string> parts(1);
            for (const char *p = i + 1 < argc ? argv[++i] : ""; *p; p++) {
                if (*p == ',')
                    parts.emplace_back();
                else
                    parts.back() += *p;
            }
            auto word = [](const string &w, const char *const *names, int n) {
                for (int k = 0; k < n; k++)
                    if (w == names[k]) return k;
                return -1;
            };
            auto number = [](const string &w) { // 1..99 from digits alone, else -1
                if (w.empty() || w.size() > 2) return -1;
                for (char c : w)
                    if (!isdigit((unsigned char)c)) return -1;
                return atoi(w.c_str());
            };
            bool clean = parts.size() >= 2 && parts.size() <= 5;
            if (clean) {
                morph_args[0] = word(parts[0], ops, 7);
                morph_args[1] = number(parts[1]);
                morph_args[2] = parts.size() > 2 ? number(parts[2]) : morph_args[1];
                morph_args[3] = parts.size() > 3 ? word(parts[3], shapes, 3) : CANNY_HIP_MORPH_RECT;
                morph_args[4] = parts.size() > 4 ? number(parts[4]) : 1;
                for (int k = 1; k <= 2; k++)
                    clean = clean && morph_args[k] >= 1 && morph_args[k] <= CANNY_HIP_MORPH_MAX_EXTENT && (morph_args[k] & 1);
                clean = clean && morph_args[0] >= 0 && morph_args[3] >= 0 && morph_args[4] >= 1 &&
                        morph_args[4] <= CANNY_HIP_MORPH_MAX_ITERATIONS;
            }
            if (!clean) {
                fprintf(stderr, "ERROR: -z expects op,kw[,kh[,shape[,iterations]]]: op erode, dilate, open, close, gradient, tophat or "
                                "blackhat, kw and kh odd in 1..31, shape rect, cross or ellipse, iterations 1..16\n");
                exit(2);
            }
            want_morph = true;
        } else if (arg == "-G") {
            // op,kw[,kh[,shape[,iterations[,border]]]]: words and whole integers, nothing empty, nothing behind the last one
            static const char *const ops[] = {"erode", "dilate", "open", "close", "gradient", "tophat", "blackhat", "median"};
            static const char *const shapes[] = {"rect", "cross", "ellipse"};
            vector<string> parts(1);
            for (const char *p = i + 1 < argc ? argv[++i] : ""; *p; p++) {
                if (*p == ',')
                    parts.emplace_back();
                else
                    parts.back() += *p;
            }
            auto word = [](const string &w, const char *const *names, int n) {
                for (int k = 0; k < n; k++)
                    if (w == names[k]) return k;
                return -1;
            };
            auto number = [](const string &w, size_t digits) { // from digits alone, else -1
                if (w.empty() || w.size() > digits) return -1;
                for (char c : w)
                    if (!isdigit((unsigned char)c)) return -1;
                return atoi(w.c_str());
            };
            bool clean = parts.size() >= 2 && parts.size() <= 6;
            if (clean) {
                gray_args[0] = word(parts[0], ops, 8);
                const bool median = gray_args[0] == CANNY_HIP_GRAY_MEDIAN;
                gray_args[1] = number(parts[1], 2);
                gray_args[2] = parts.size() > 2 ? number(parts[2], 2) : gray_args[1];
                gray_args[3] = parts.size() > 3 ? word(parts[3], shapes, 3) : CANNY_HIP_MORPH_RECT;
                gray_args[4] = parts.size() > 4 ? number(parts[4], 2) : 1;
                gray_args[5] = median ? CANNY_HIP_GRAY_BORDER_REPLICATE : CANNY_HIP_GRAY_BORDER_NEUTRAL, gray_args[6] = 0;
                if (parts.size() > 5) {
                    if (parts[5] == "neutral") {
                        gray_args[5] = CANNY_HIP_GRAY_BORDER_NEUTRAL;
                    } else if (parts[5] == "replicate") {
                        gray_args[5] = CANNY_HIP_GRAY_BORDER_REPLICATE;
                    } else {
                        gray_args[5] = CANNY_HIP_GRAY_BORDER_CONSTANT, gray_args[6] = number(parts[5], 3);
                        clean = gray_args[6] >= 0 && gray_args[6] <= 255;
                    }
                }
                for (int k = 1; k <= 2; k++)
                    clean = clean && gray_args[k] >= 1 && gray_args[k] <= CANNY_HIP_MORPH_MAX_EXTENT && (gray_args[k] & 1);
                clean = clean && gray_args[0] >= 0 && gray_args[3] >= 0 && gray_args[4] >= 1 &&
                        gray_args[4] <= CANNY_HIP_MORPH_MAX_ITERATIONS;
                if (median)
                    clean = clean && (gray_args[1] == 3 || gray_args[1] == 5) && gray_args[2] == gray_args[1] &&
                            gray_args[3] == CANNY_HIP_MORPH_RECT && gray_args[5] != CANNY_HIP_GRAY_BORDER_NEUTRAL;
            }
            if (!clean) {
                fprintf(stderr, "ERROR: -G expects op,kw[,kh[,shape[,iterations[,border]]]]: op erode, dilate, open, close, gradient, "
                                "tophat, blackhat or median, kw and kh odd in 1..31 (median: 3 or 5, square, rect), shape rect, cross "
                                "or ellipse, iterations 1..16, border neutral (not for median), replicate or 0..255\n");
                exit(2);
            }
            want_gray = true;
        } else if (arg == "-P") {
            // levels[,up]: a whole integer 1..15 of digits alone and the word up, nothing empty, nothing behind the last one
            const string value = i + 1 < argc ? argv[++i] : "";
            const size_t comma = value.find(',');
            const string number = value.substr(0, comma);
            bool clean = !number.empty() && number.size() <= 2 && (comma == string::npos || value.substr(comma + 1) == "up");
            for (char c : number) clean = clean && isdigit((unsigned char)c);
            if (clean) pyramid_levels = atoi(number.c_str());
            clean = clean && pyramid_levels >= 1 && pyramid_levels <= CANNY_HIP_PYR_MAX_LEVELS;
            if (!clean) {
                fprintf(stderr, "ERROR: -P expects levels[,up]: levels 1..15 (at most ceil(log2(max(height, width)))), up to also bring "
                                "level 1 back to the frame's size\n");
                exit(2);
            }
            want_pyramid = true, pyramid_up = comma != string::npos;
        } else if (arg == "-a") {
            // method[,thr_or_c[,kw[,kh[,invert]]]]: a word and whole integers, nothing empty, nothing behind the last one
            static const char *const methods[] = {"fixed", "otsu", "mean"};
            vector<string> parts(1);
            for (const char *p = i + 1 < argc ? argv[++i] : ""; *p; p++) {
                if (*p == ',')
                    parts.emplace_back();
                else
                    parts.back() += *p;
            }
            auto number = [](const string &w, int &v) { // -999..999 from an optional sign and digits alone
                const size_t d = !w.empty() && w[0] == '-' ? 1 : 0;
                if (w.size() == d || w.size() > d + 3) return false;
                for (size_t k = d; k < w.size(); k++)
                    if (!isdigit((unsigned char)w[k])) return false;
                v = atoi(w.c_str());
                return true;
            };
            bool clean = parts.size() >= 1 && parts.size() <= 5;
            if (clean) {
                bin_args[0] = -1;
                for (int k = 0; k < 3; k++)
                    if (parts[0] == methods[k]) bin_args[0] = k;
                bin_args[1] = bin_args[0] == CANNY_HIP_BIN_FIXED ? 127 : (bin_args[0] == CANNY_HIP_BIN_OTSU ? 0 : 7);
                clean = bin_args[0] >= 0;
                for (size_t k = 1; k < parts.size(); k++) clean = clean && number(parts[k], bin_args[k]);
                if (parts.size() < 4) bin_args[3] = bin_args[2];
                if (clean && bin_args[0] == CANNY_HIP_BIN_FIXED) clean = bin_args[1] >= -1 && bin_args[1] <= 255;
                if (clean && bin_args[0] == CANNY_HIP_BIN_ADAPTIVE_MEAN) {
                    clean = bin_args[1] >= -255 && bin_args[1] <= 255;
                    for (int k = 2; k <= 3; k++)
                        clean = clean && bin_args[k] >= 3 && bin_args[k] <= CANNY_HIP_BIN_MAX_EXTENT && (bin_args[k] & 1);
                }
                clean = clean && (bin_args[4] == 0 || bin_args[4] == 1);
            }
            if (!clean) {
                fprintf(stderr, "ERROR: -a expects method[,thr_or_c[,kw[,kh[,invert]]]]: method fixed (thr -1..255), otsu or mean (c "
                                "-255..255, kw and kh odd in 3..255), invert 0 or 1\n");
                exit(2);
            }
            want_binarize = true;
        } else if (arg == "-v") {
            // method[,max_iterations]: a word and a whole number, nothing empty, nothing behind it
            const string spec = i + 1 < argc ? argv[++i] : "";
            const size_t comma = spec.find(',');
            const string word = spec.substr(0, comma), num = comma == string::npos ? string("0") : spec.substr(comma + 1);
            thin_args[0] = word == "guohall" ? CANNY_HIP_THIN_GUOHALL : (word == "zhangsuen" ? CANNY_HIP_THIN_ZHANGSUEN : -1);
            bool clean = thin_args[0] >= 0 && !num.empty() && num.size() <= 5;
            for (char c : num) clean = clean && isdigit((unsigned char)c);
            if (clean) thin_args[1] = atoi(num.c_str());
            if (!clean || thin_args[1] > CANNY_HIP_THIN_MAX_ITERATIONS) {
                fprintf(stderr, "ERROR: -v expects method[,max_iterations]: method guohall or zhangsuen, max_iterations 0..16384 "
                                "(0: to the fixed point)\n");
                exit(2);
            }
            want_thin = true;
        } else if (arg == "-R") {
            // op[,connectivity[,thr]]: a word, 4 or 8, and for seeded a whole number -1..255; nothing empty, nothing behind it
            static const char *const ops[] = {"seeded", "fill", "clear"};
            vector<string> parts(1);
            for (const char *p = i + 1 < argc ? argv[++i] : ""; *p; p++) {
                if (*p == ',')
                    parts.emplace_back();
                else
                    parts.back() += *p;
            }
            recon_args[0] = -1, recon_args[1] = 8, recon_thr_given = false;
            for (int k = 0; k < 3; k++)
                if (parts[0] == ops[k]) recon_args[0] = k;
            bool clean = recon_args[0] >= 0 && parts.size() <= (recon_args[0] == CANNY_HIP_RECON_SEEDED ? 3u : 2u);
            if (clean && parts.size() >= 2) {
                clean = parts[1] == "4" || parts[1] == "8";
                recon_args[1] = parts[1] == "4" ? 4 : 8;
            }
            if (clean && parts.size() == 3) {
                const string &t = parts[2];
                const size_t d = !t.empty() && t[0] == '-' ? 1 : 0;
                clean = t.size() > d && t.size() <= d + 3;
                for (size_t k = d; k < t.size(); k++) clean = clean && isdigit((unsigned char)t[k]);
                if (clean) recon_args[2] = atoi(t.c_str());
                clean = clean && recon_args[2] >= -1 && recon_args[2] <= 255;
                recon_thr_given = clean;
            }
            if (clean && recon_args[0] == CANNY_HIP_RECON_SEEDED) clean = recon_thr_given;
            if (!clean) {
                fprintf(stderr, "ERROR: -R expects op[,connectivity[,thr]]: op fill, clear or seeded, connectivity 4 or 8, and for "
                                "seeded (with -a fixed,...) the marker's threshold thr -1..255\n");
                exit(2);
            }
            want_recon = true;
        } else if (arg == "-w" && i + 1 < argc) {
            char tail = 0; // a whole integer only
            if (sscanf(argv[++i], "%d%c", &curve_min_length, &tail) != 1) {
                fprintf(stderr, "ERROR: -w expects min_length\n");
                exit(2);
            }
            want_curves = true;
        } else if (arg == "-e") {
            want_edgels = true;
        } else if (arg == "-n" && i + 1 < argc) {
            if (sscanf(argv[++i], "%dx%d", &width, &height) != 2 || width < 2 || height < 2) {
                fprintf(stderr, "ERROR: -n expects WIDTHxHEIGHT\n");
                exit(0);
            }
        } else {
            values.push_back(arg);
        }
    }

    if (want_segments && !want_lines) {
        fprintf(stderr, "ERROR: -g needs the lines of -l rho,theta_degrees,threshold[,lines_max]\n");
        exit(2);
    }
    if (fit_options >= 0 && !(want_lines && want_segments)) {
        fprintf(stderr, "ERROR: -f needs the segments of -l rho,theta_degrees,threshold[,lines_max] and -g min_length,max_gap[,exclusive]\n");
        exit(2);
    }
    if (want_circle_fits && !want_circles) {
        fprintf(stderr, "ERROR: -k needs the circles of -r min_radius,max_radius,threshold,support[,min_dist[,cell_shift]]\n");
        exit(2);
    }
    if (desc_options >= 0 && !want_corners) {
        fprintf(stderr, "ERROR: -j needs the corners of -q quality_q16,min_dist,corners_max[,block[,k_q8]]\n");
        exit(2);
    }
    if (want_polygons && !want_contours) {
        fprintf(stderr, "ERROR: -y needs the contours of -t\n");
        exit(2);
    }
    if (want_shapes && !want_contours) {
        fprintf(stderr, "ERROR: -u needs the contours of -t\n");
        exit(2);
    }
    if (want_recon && recon_args[0] == CANNY_HIP_RECON_SEEDED && !(want_binarize && bin_args[0] == CANNY_HIP_BIN_FIXED)) {
        fprintf(stderr, "ERROR: -R seeded needs -a fixed,...: its marker is the same plane binarized at thr\n");
        exit(2);
    }
    if (values.size() != 3) {
        fprintf(stderr, "USAGE: %s sigma minVal maxVal\n", argv[0]);
        fprintf(stderr, "   sigma: Standard deviation used for the gaussian blurring kernel\n");
        fprintf(stderr, "   minVal: The minimum threshold value used for hysteresis\n");
        fprintf(stderr, "           Must be in the range of [0,255]\n");
        fprintf(stderr, "   maxVal: The maximum threshold value used for hysteresis\n");
        fprintf(stderr, "           Must be in the range of [0,255]\n");
        fprintf(stderr, "   -c: use the GPU entry point (cuda_canny)   -s: write every step\n");
        fprintf(stderr, "   -i frame: input frame (binary PGM, binary PPM or baseline JPEG)   -n WxH: synthetic frame size   -o dir: output dir\n");
        fprintf(stderr, "   -p: write PNG files instead of PGM\n");
        fprintf(stderr, "   -b dir: run every .pgm / .jpg of dir as one batch, write <name>_edges.pgm\n");
        fprintf(stderr, "   -l rho,theta_degrees,threshold[,lines_max]: Hough lines of the edge map -> canny_lines.txt in the -o dir\n");
        fprintf(stderr, "   -g min_length,max_gap[,exclusive]: with -l, the segments along the lines -> canny_segments.txt in the -o dir\n");
        fprintf(stderr, "   -f options: with -l and -g, the sub-pixel line fit of every segment (options 0..3: 1 = gate by gradient\n");
        fprintf(stderr, "       direction, 2 = refined edgels only), one \"x0 y0 x1 y1 cx cy dx dy n rms maxd degenerate\" line each (pixels)\n");
        fprintf(stderr, "       -> canny_line_fits.txt in the -o dir\n");
        fprintf(stderr, "   -m min_area: connected components of the edge map with at least min_area pixels -> canny_components.txt,\n");
        fprintf(stderr, "                canny_kept.pgm in the -o dir\n");
        fprintf(stderr, "   -t: outer contour chain of every component with at least min_area (-m, default 1) pixels, one\n");
        fprintf(stderr, "       \"label n x0 y0 x1 y1 ...\" line each -> canny_contours.txt in the -o dir\n");
        fprintf(stderr, "   -w min_length: edge curves of the edge map with at least min_length points (every edge pixel once, in order\n");
        fprintf(stderr, "       along its curve, split at junctions), one \"start end points flags x0 y0 x1 y1 ...\" line each ->\n");
        fprintf(stderr, "       canny_curves.txt in the -o dir\n");
        fprintf(stderr, "   -y epsilon[,ratio]: with -t, the polygon of every contour at a tolerance of epsilon pixels plus ratio times\n");
        fprintf(stderr, "       its length, one \"frame record vertices length area2 convex x0 y0 x1 y1 ...\" line each (length in 1/256\n");
        fprintf(stderr, "       pixel, area2 twice the area) -> canny_polygons.txt in the -o dir\n");
        fprintf(stderr, "   -u: with -t, the moments, convex hull and minimum-area rectangle of every contour, one \"frame record points\n");
        fprintf(stderr, "       hull_vertices area2 hull_area2 rect_edge rect_along_min rect_along_max rect_across rect_len2 x0 y0 x1 y1 ...\"\n");
        fprintf(stderr, "       line each (the pairs are the hull) -> canny_shapes.txt in the -o dir\n");
        fprintf(stderr, "   -r min_radius,max_radius,threshold,support[,min_dist[,cell_shift]]: circles of the edge map, one\n");
        fprintf(stderr, "       \"frame x y radius votes support\" line each -> canny_circles.txt in the -o dir\n");
        fprintf(stderr, "   -k band,trim_q8[,options]: with -r, the sub-pixel circle fit of every circle (band 0..4 bins each side, trim_q8 in\n");
        fprintf(stderr, "       1/256 px or 0, options 0..3: 1 = gate by gradient direction, 2 = refined edgels only), one \"frame cx cy r n rms\n");
        fprintf(stderr, "       maxd sectors trim_failed degenerate\" line each (pixels; sectors in hex) -> canny_circle_fits.txt in the -o dir\n");
        fprintf(stderr, "   -x a.pgm[:b.pgm...],trunc_q4,max_mean_q4,min_dist: chamfer matching of the edge map against the shapes of the\n");
        fprintf(stderr, "       PGM files (non-zero pixels, anchored at the centre; costs in 1/16 px), one \"frame x y template score mean\"\n");
        fprintf(stderr, "       line per match (mean in pixels) -> canny_matches.txt in the -o dir\n");
        fprintf(stderr, "   -q quality_q16,min_dist,corners_max[,block[,k_q8]]: corners of the smoothed plane (Shi-Tomasi; with k_q8 Harris,\n");
        fprintf(stderr, "       k in 1/256), one \"frame x y response rank\" line each -> canny_corners.txt in the -o dir\n");
        fprintf(stderr, "   -j upright|steered: with -q, the 256-bit descriptor of every corner (steered: turned to the patch's centroid),\n");
        fprintf(stderr, "       one \"x y k border\" and 64 hex digits each -> canny_descriptors.txt in the -o dir\n");
        fprintf(stderr, "   -z op,kw[,kh[,shape[,iterations]]]: binary morphology of the edge map (erode, dilate, open, close, gradient,\n");
        fprintf(stderr, "       tophat, blackhat; kw, kh odd 1..31; rect, cross, ellipse; 1..16 iterations) -> canny_morph.pgm in the -o dir\n");
        fprintf(stderr, "   -G op,kw[,kh[,shape[,iterations[,border]]]]: a grey-level operator on the input frame (the words of -z, or median\n");
        fprintf(stderr, "       with kw 3 or 5; border neutral, replicate or 0..255) -> canny_gray.pgm in the -o dir; with -a also the\n");
        fprintf(stderr, "       binarization of that plane, on the device -> canny_gray_binary.pgm\n");
        fprintf(stderr, "   -P levels[,up]: the pyramid of the input frame on the device (pyrDown: 5 x 5 binomial, every second pixel; levels\n");
        fprintf(stderr, "       1..15) -> canny_pyr1.pgm .. canny_pyr<levels>.pgm in the -o dir; with up also level 1 brought back to the\n");
        fprintf(stderr, "       frame's size (pyrUp) -> canny_pyr_up.pgm\n");
        fprintf(stderr, "   -a method[,thr_or_c[,kw[,kh[,invert]]]]: the input frame binarized (fixed: thr -1..255; otsu: the frame's own\n");
        fprintf(stderr, "       threshold, printed; mean: adaptive, offset c, window kw x kh odd 3..255; invert 0 or 1) -> canny_binary.pgm in the -o dir\n");
        fprintf(stderr, "   -v method[,max_iterations]: the edge map -- with -a the binarized frame, on the device -- thinned to a one-pixel\n");
        fprintf(stderr, "       skeleton (guohall or zhangsuen; 0..16384 iterations, 0: to the fixed point) -> canny_thin.pgm in the -o dir\n");
        fprintf(stderr, "   -R op[,connectivity[,thr]]: the edge map -- with -a the binarized frame, on the device -- reconstructed: fill (holes\n");
        fprintf(stderr, "       filled), clear (blobs at the frame border dropped) or seeded (with -a fixed,lo: the blobs that hold a pixel above\n");
        fprintf(stderr, "       thr, hysteresis thresholding of the frame); connectivity 4 or 8 -> canny_reconstruct.pgm in the -o dir\n");
        fprintf(stderr, "   -d: distance of every pixel to the nearest edge pixel, min(255, floor) -> canny_dist.pgm in the -o dir\n");
        fprintf(stderr, "   -e: sub-pixel edgel of every edge pixel, one \"x y gx gy mag dir refined\" line each (x, y in pixels to three\n");
        fprintf(stderr, "       decimals, mag in grey levels, dir 0..3) -> canny_edgels.txt in the -o dir\n");
        exit(0);
    }

    try {
        sigma = stof(values[0]);
        minVal = stoi(values[1]);
        maxVal = stoi(values[2]);
    } catch (const exception &) {
        fprintf(stderr, "ERROR: sigma, minVal and maxVal must be numbers\n");
        exit(0);
    }

    if (maxVal <= minVal) {
        fprintf(stderr, "ERROR: minVal must be less than maxVal\n");
        exit(0);
    }
    if (minVal < 0 or minVal > 255) {
        fprintf(stderr, "ERROR: minVal must be in the range of [0,255]");
        exit(0);
    }
    if (maxVal < 0 or maxVal > 255) {
        fprintf(stderr, "ERROR: maxVal must be in the range of [0,255]");
        exit(0);
    }

    if (!batch_dir.empty()) return run_batch(batch_dir, outdir, sigma, minVal, maxVal);

    vector<unsigned char> frame;
    if (!input.empty()) {
        if (!read_frame(input, frame, height, width)) {
            cout << "ERROR: Failed to open " << input << endl;
            return -1;
        }
    } else {
        synthetic_frame(frame, height, width);
    }
    if (!outdir.empty()) setenv("CANNY_OUTPUT_DIR", outdir.c_str(), 1);
    if (png_output) setenv("CANNY_OUTPUT_FORMAT", "png", 1);
    if (show_steps && is_ppm(input)) { // the converted plane, the step the reference's cvtColor did
        const string path = (outdir.empty() ? string(".") : outdir) + "/canny_step0_gray" + (png_output ? ".png" : ".pgm");
        if (canny_frames_write_gray(path.c_str(), frame.data(), height, width))
            cerr << "WARNING: cannot write " << path << "\n";
    }

    try {
        if (use_gpu_entry)
            cuda_canny(frame.data(), sigma, minVal, maxVal, height, width, show_steps);
        else
            canny(frame.data(), sigma, minVal, maxVal, height, width, show_steps);
    } catch (const exception &e) {
        fprintf(stderr, "ERROR: %s\n", e.what());
        return 1;
    }
    if (want_components) {
        const int rc = run_components(frame, height, width, sigma, minVal, maxVal, min_area, outdir);
        if (rc) return rc;
    }
    if (want_contours) {
        const int rc = run_contours(frame, height, width, sigma, minVal, maxVal, min_area, outdir);
        if (rc) return rc;
    }
    if (want_curves) {
        const int rc = run_curves(frame, height, width, sigma, minVal, maxVal, curve_min_length, outdir);
        if (rc) return rc;
    }
    if (want_polygons) {
        const int rc = run_polygons(frame, height, width, sigma, minVal, maxVal, min_area, polygon_epsilon_q8,
                                    polygon_ratio_q16, outdir);
        if (rc) return rc;
    }
    if (want_shapes) {
        const int rc = run_shapes(frame, height, width, sigma, minVal, maxVal, min_area, outdir);
        if (rc) return rc;
    }
    if (want_edgels) {
        const int rc = run_edgels(frame, height, width, sigma, minVal, maxVal, outdir);
        if (rc) return rc;
    }
    if (want_morph) {
        const int rc = run_morph(frame, height, width, sigma, minVal, maxVal, morph_args, outdir);
        if (rc) return rc;
    }
    if (want_binarize) {
        const int rc = run_binarize(frame, height, width, bin_args, outdir);
        if (rc) return rc;
    }
    if (want_gray) {
        const int rc = run_gray_morph(frame, height, width, gray_args, want_binarize ? bin_args : nullptr, outdir);
        if (rc) return rc;
    }
    if (want_pyramid) {
        const int rc = run_pyramid(frame, height, width, pyramid_levels, pyramid_up, outdir);
        if (rc) return rc;
    }
    if (want_thin) {
        const int rc = run_thin(frame, height, width, sigma, minVal, maxVal, want_binarize ? bin_args : nullptr, thin_args, outdir);
        if (rc) return rc;
    }
    if (want_recon) {
        const int rc = run_reconstruct(frame, height, width, sigma, minVal, maxVal, want_binarize ? bin_args : nullptr, recon_args,
                                       outdir);
        if (rc) return rc;
    }
    if (want_dist) {
        const int rc = run_edt(frame, height, width, sigma, minVal, maxVal, outdir);
        if (rc) return rc;
    }
    if (!chamfer_shapes.empty()) {
        const int rc = run_chamfer(frame, height, width, sigma, minVal, maxVal, chamfer_shapes, chamfer_args, outdir);
        if (rc) return rc;
    }
    if (want_corners && desc_options >= 0) {
        const int rc = run_descriptors(frame, height, width, sigma, minVal, maxVal, corner_args, desc_options, outdir);
        if (rc) return rc;
    } else if (want_corners) {
        const int rc = run_corners(frame, height, width, sigma, minVal, maxVal, corner_args, outdir);
        if (rc) return rc;
    }
    if (want_circles) {
        const int rc = run_circles(frame, height, width, sigma, minVal, maxVal, circle_args, want_circle_fits ? circle_fit_args : nullptr,
                                   outdir);
        if (rc) return rc;
    }
    if (want_lines && want_segments)
        return run_segments(frame, height, width, sigma, minVal, maxVal, line_rho, line_theta_deg, line_threshold, lines_max,
                            seg_min_length, seg_max_gap, seg_exclusive, fit_options, outdir);
    if (want_lines)
        return run_hough(frame, height, width, sigma, minVal, maxVal, line_rho, line_theta_deg, line_threshold, lines_max,
                         outdir);
    return 0;
}
