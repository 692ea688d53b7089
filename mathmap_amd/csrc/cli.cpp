// `mathmap` command line on the HIP engine: same options, defaults and messages as the
// reference's mathmap_cmdline.c:423-895 (usage text :423-452, option table :489-522,
// -D handling :756-796, render loop :798-871), rendering through libmathmap_hip.so.
//
// PNG input/output uses a small zlib-based codec (the reference links libpng through
// rwimg/; only zlib is available here): reads 8/16-bit grey, grey+alpha, RGB, RGBA and
// palette PNGs (non-interlaced) into RGB8 -- alpha is discarded exactly like
// rwimg/rwpng.c:104-158 does -- and writes RGB8 (rwpng.c:172-251: the alpha channel of the
// RGBA render is dropped).
#include <getopt.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mmhip.h"

namespace {

int cache_size = 8;

void usage() {
    printf("Usage:\n"
           "  mathmap --version\n"
           "      print out version number\n"
           "  mathmap --help\n"
           "      print this help text\n"
           "  mathmap [option ...] [<script>] <outfile>\n"
           "      transform one or more inputs with <script> and write\n"
           "      the result to <outfile>\n"
           "  mathmap --htmldoc [<script>] <outfile>\n"
           "      outputs HTML documentation for the filters in\n"
           "      the script to <outfile>\n"
           "Options:\n"
           "  -f, --script-file=FILENAME  read script from FILENAME\n"
           "  -D<name>=<value>            define user value\n"
           "  -F, --frames=NUM            render NUM animation frames (t = frame/NUM);\n"
           "                              <outfile> may contain %%d for the frame number\n"
           "  -i, --intersampling         use intersampling\n"
           "  -o, --oversampling          use oversampling\n"
           "  -s, --size=WIDTHxHEIGHT     sets the output image size\n"
           "  -c, --cache=NUM             cache NUM input images (default %d)\n"
           "  -g, --generator=GEN         generate plug-in code with GEN\n"
           "Extensions of the HIP command line:\n"
           "      --gauss-mode=MODE       gaussian_blur arithmetic: exact (default, the\n"
           "                              reference's values) or tolerance (faster, RGBA8\n"
           "                              output within 1 per channel of exact)\n"
           "      --input-frames=NUM      an input image whose file name contains a\n"
           "                              conversion like %%d is a sequence: frames 0 to\n"
           "                              NUM-1 are read from the files so named (all of\n"
           "                              one size) and in(xy, n) reads frame n; with -F,\n"
           "                              in(xy, frame) processes a clip frame by frame\n"
           "      --native-input-frame=MODE  which frame of an --input-frames sequence\n"
           "                              gaussian_blur, render() and convolve read:\n"
           "                              zero (default, like the reference) or current\n"
           "                              (the frame being rendered)\n"
           "      --batch-frames=NUM      with -F, render NUM frames per batched GPU\n"
           "                              launch (default 1: frame by frame); the files\n"
           "                              are the same\n"
           "      --shutter-samples=K     with -F, motion blur: every frame is the mean of\n"
           "                              K (1 to 256) renders spread over the shutter\n"
           "                              time, averaged on the GPU before the bytes are\n"
           "                              made; not combined with -o\n"
           "      --shutter=FRACTION      the shutter time as a fraction of the frame\n"
           "                              interval (default 0.5): sub-sample j is rendered\n"
           "                              at t = frame/NUM + FRACTION/NUM * j/K\n"
           "      --shutter-mode=MODE     how the K renders are averaged: maps (default,\n"
           "                              float maps in device memory) or fused (summed in\n"
           "                              the pixel kernel); the files are the same\n"
           "      --aa=N | SXxSY          anti-aliasing: every pixel is the mean of\n"
           "                              an N x N (or SX x SY, 1 to 8 each) grid of renders\n"
           "                              inside its footprint, averaged in float on the\n"
           "                              GPU; combines with --shutter-samples (K * SX * SY\n"
           "                              at most 256), --shutter-mode and --batch-frames;\n"
           "                              not combined with -o\n"
           "      --aa-threshold=T        with --aa, adaptive anti-aliasing: only pixels\n"
           "                              whose clamped value differs by more than T from\n"
           "                              one of their 8 neighbours in a single-sample\n"
           "                              render get the grid; the others keep that\n"
           "                              render's value; not combined with -o or\n"
           "                              --shutter-samples\n"
           "      --aa-refine=MODE        with --aa-threshold, how the refined pixels are\n"
           "                              rendered: list (default: they alone, where the\n"
           "                              filter allows it) or select (the whole grid\n"
           "                              render, then the choice); the files are the same\n"
           "      --aa-filter=NAME[:RADIUS]\n"
           "                              with --aa (which may be --aa=1), weight the\n"
           "                              grid's renders with a reconstruction filter that\n"
           "                              reaches into the neighbour pixels: box, tent,\n"
           "                              gaussian or mitchell, RADIUS in pixels from 0.5\n"
           "                              to 4 (default 0.5, 1, 1.5 and 2); not combined\n"
           "                              with -o, --aa-threshold or --shutter-mode=fused\n"
           "  <outfile> ending in .y4m    write all -F frames (-F 1 too) to one YUV4MPEG2\n"
           "                              file, planar Y'CbCr 4:2:0 converted on the GPU\n"
           "                              (C420jpeg chroma siting), which video encoders\n"
           "                              read; an <outfile> of - writes that stream to\n"
           "                              standard output, for a pipe; --batch-frames is then\n"
           "                              by default what fits in 1 GiB of device memory\n"
           "      --yuv-matrix=MATRIX     with a .y4m output: bt709 (default) or bt601\n"
           "      --yuv-range=RANGE       with a .y4m output: limited (default, Y 16-235)\n"
           "                              or full (0-255)\n"
           "      --fps=N[:D]             with a .y4m output: the frame rate N/D written\n"
           "                              to the header (default 25)\n"
           "      --pixel-format=FORMAT   with a .y4m output: yuv420p (default, 8-bit\n"
           "                              samples converted from the RGBA8 frames) or\n"
           "                              yuv420p10 (C420p10: 10-bit samples in 16-bit\n"
           "                              little-endian words, converted from the float\n"
           "                              pixels before any 8-bit store; Y 64-940 at\n"
           "                              limited range); yuv420p10 is not combined with -o\n"
           "  -D<name>=FILE.y4m           an input image whose file name ends in .y4m, or is -\n"
           "                              (standard input, for one image at most), is a\n"
           "                              YUV4MPEG2 stream of 8-bit 4:2:0 frames: all its\n"
           "                              frames (--input-frames=NUM: the first NUM) are bound\n"
           "                              as a sequence and expanded to RGB on the GPU; a\n"
           "                              stream whose header says C420p10 (10-bit samples in\n"
           "                              16-bit little-endian words) is expanded to float32\n"
           "                              pixels instead, unclamped and with no 8-bit step,\n"
           "                              and the filter is compiled for float32 inputs\n"
           "                              (native filters like gaussian_blur do not read\n"
           "                              such an image); without\n"
           "                              -s the size is the stream's, without -F every input\n"
           "                              frame is rendered, and a .y4m output without --fps\n"
           "                              takes the stream's frame rate; in(xy, frame)\n"
           "                              processes the video frame by frame\n"
           "      --input-yuv-matrix=MATRIX  with a .y4m input: bt709 (default) or bt601\n"
           "      --input-yuv-range=RANGE with a .y4m input: limited or full (default: the\n"
           "                              stream's XCOLORRANGE, else limited)\n"
           "      --input-chroma=MODE     with a .y4m input: bilinear (default, chroma\n"
           "                              interpolated between the 2 x 2 blocks' centres) or\n"
           "                              replicate (a block's four pixels share its chroma)\n"
           "      --chroma-siting=SITING  with a .y4m output: center (default, a chroma sample\n"
           "                              at the centre of its 2 x 2 block, C420jpeg) or left\n"
           "                              (co-sited with the even luma column, what H.264,\n"
           "                              HEVC and AV1 encoders assume; an 8-bit stream is\n"
           "                              tagged C420mpeg2, C420p10 has no tag for it)\n"
           "      --input-chroma-siting=SITING  with a .y4m input: center (default), left\n"
           "                              (C420mpeg2, what video decoders emit) or auto (left\n"
           "                              where the stream's header says C420mpeg2, else\n"
           "                              center); replicate chroma ignores it\n"
           "\n"
           "Report bugs and suggestions to schani@complang.tuwien.ac.at\n",
           cache_size);
}

// ---- PNG ------------------------------------------------------------------------------------
uint32_t be32(const unsigned char *p) { return ((uint32_t)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

bool read_png(const char *path, std::vector<unsigned char> &rgb, int &w, int &h) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::vector<unsigned char> data;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (data.size() < 8 || memcmp(data.data(), sig, 8)) return false;
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<unsigned char> idat, plte;
    size_t p = 8;
    while (p + 12 <= data.size()) {
        uint32_t len = be32(&data[p]);
        const unsigned char *type = &data[p + 4];
        const unsigned char *body = &data[p + 8];
        if (p + 12 + len > data.size()) return false;
        if (!memcmp(type, "IHDR", 4)) {
            w = (int)be32(body); h = (int)be32(body + 4); depth = body[8]; ctype = body[9]; interlace = body[12];
        } else if (!memcmp(type, "PLTE", 4)) plte.assign(body, body + len);
        else if (!memcmp(type, "IDAT", 4)) idat.insert(idat.end(), body, body + len);
        else if (!memcmp(type, "IEND", 4)) break;
        p += 12 + len;
    }
    if (w <= 0 || h <= 0 || interlace || (depth != 8 && depth != 16)) return false;
    int channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!channels || (ctype == 3 && depth != 8)) return false;
    int bpp = channels * depth / 8;
    size_t stride = (size_t)w * bpp;
    std::vector<unsigned char> raw((stride + 1) * h);
    uLongf rawlen = raw.size();
    if (uncompress(raw.data(), &rawlen, idat.data(), idat.size()) != Z_OK || rawlen != raw.size()) return false;
    std::vector<unsigned char> img(stride * h);
    for (int y = 0; y < h; ++y) {
        const unsigned char *src = &raw[(stride + 1) * y];
        unsigned char *dst = &img[stride * y];
        const unsigned char *up = y ? &img[stride * (y - 1)] : nullptr;
        int ft = src[0];
        for (size_t i = 0; i < stride; ++i) {
            int a = i >= (size_t)bpp ? dst[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= (size_t)bpp) ? up[i - bpp] : 0;
            int x = src[i + 1], v;
            switch (ft) {
                case 0: v = x; break;
                case 1: v = x + a; break;
                case 2: v = x + b; break;
                case 3: v = x + ((a + b) >> 1); break;
                case 4: {
                    int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
                    v = x + ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
                    break;
                }
                default: return false;
            }
            dst[i] = (unsigned char)v;
        }
    }
    rgb.resize((size_t)w * h * 3);
    int step = depth / 8;
    for (size_t i = 0; i < (size_t)w * h; ++i) {
        const unsigned char *s = &img[i * bpp];
        unsigned char *d = &rgb[i * 3];
        switch (ctype) {
            case 0: case 4: d[0] = d[1] = d[2] = s[0]; break;
            case 2: case 6: d[0] = s[0]; d[1] = s[step]; d[2] = s[2 * step]; break;
            case 3:
                if ((size_t)s[0] * 3 + 2 >= plte.size()) return false;
                d[0] = plte[s[0] * 3]; d[1] = plte[s[0] * 3 + 1]; d[2] = plte[s[0] * 3 + 2];
                break;
        }
    }
    return true;
}

void put_chunk(FILE *f, const char *type, const unsigned char *body, size_t len) {
    unsigned char hdr[8] = {(unsigned char)(len >> 24), (unsigned char)(len >> 16), (unsigned char)(len >> 8),
                            (unsigned char)len, (unsigned char)type[0], (unsigned char)type[1], (unsigned char)type[2],
                            (unsigned char)type[3]};
    fwrite(hdr, 1, 8, f);
    if (len) fwrite(body, 1, len, f);
    uLong crc = crc32(0, hdr + 4, 4);
    if (len) crc = crc32(crc, body, (uInt)len);
    unsigned char c[4] = {(unsigned char)(crc >> 24), (unsigned char)(crc >> 16), (unsigned char)(crc >> 8), (unsigned char)crc};
    fwrite(c, 1, 4, f);
}

bool write_png_rgb(const char *path, const unsigned char *rgba, int w, int h) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    fwrite(sig, 1, 8, f);
    unsigned char ihdr[13] = {(unsigned char)(w >> 24), (unsigned char)(w >> 16), (unsigned char)(w >> 8), (unsigned char)w,
                              (unsigned char)(h >> 24), (unsigned char)(h >> 16), (unsigned char)(h >> 8), (unsigned char)h,
                              8, 2, 0, 0, 0};
    put_chunk(f, "IHDR", ihdr, 13);
    std::vector<unsigned char> raw(((size_t)w * 3 + 1) * h);
    for (int y = 0; y < h; ++y) {
        unsigned char *d = &raw[((size_t)w * 3 + 1) * y];
        *d++ = 0;
        const unsigned char *s = rgba + (size_t)y * w * 4;
        for (int x = 0; x < w; ++x) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d += 3; s += 4; }
    }
    uLongf clen = compressBound(raw.size());
    std::vector<unsigned char> comp(clen);
    if (compress2(comp.data(), &clen, raw.data(), raw.size(), 6) != Z_OK) { fclose(f); return false; }
    put_chunk(f, "IDAT", comp.data(), clen);
    put_chunk(f, "IEND", nullptr, 0);
    fclose(f);
    return true;
}

struct Define { std::string name, value; };

// A YUV4MPEG2 stream of 4:2:0 frames of 8 or 10 bits (mmhip_y4m_parse_stream_header states what a header may hold): its
// payloads one after the other, as mmhip_set_image_sequence_yuv420_host (bits 8) or ..._yuv420p10_host (bits 10) takes
// them.
struct Y4mStream {
    int uv = -1;      // the image user value it is bound to
    int width = 0, height = 0, fps_num = 25, fps_den = 1, range = -1, bits = 8, frames = 0;
    int siting = MMHIP_YUV_SITING_CENTER;      // what the header's C tag states (mmhip_y4m_stream_siting)
    std::vector<unsigned char> payloads;
};
bool is_y4m_name(const std::string &v) { return v == "-" || (v.size() >= 4 && v.compare(v.size() - 4, 4, ".y4m") == 0); }
// One line of at most `cap` bytes, the newline included; false at the end of the file before any byte.
bool read_line(FILE *f, std::string &line, size_t cap) {
    line.clear();
    for (int c; line.size() < cap && (c = fgetc(f)) != EOF;) {
        line.push_back((char)c);
        if (c == '\n') break;
    }
    return !line.empty();
}
// Reads the stream `name` (- is standard input), at most max_frames frames of it (0: all).  On failure `err` says why.
bool read_y4m(const std::string &name, int max_frames, Y4mStream &out, std::string &err) {
    FILE *f = name == "-" ? stdin : fopen(name.c_str(), "rb");
    if (!f) { err = "Could not read input stream `" + name + "': " + strerror(errno); return false; }
    auto done = [&](bool ok) {
        if (f != stdin) fclose(f);
        return ok;
    };
    std::string line;
    read_line(f, line, 4096);
    int header_len = 0;
    if (mmhip_y4m_parse_stream_header(line.data(), (int)line.size(), &out.width, &out.height, &out.fps_num, &out.fps_den, &out.range, &out.bits,
                                      &header_len) != 0 ||
        mmhip_y4m_stream_siting(line.data(), (int)line.size(), &out.siting) != 0) {
        err = "`" + name + "': " + mmhip_last_error();
        return done(false);
    }
    const size_t frame_bytes = (size_t)(out.bits == 10 ? mmhip_yuv420p10_frame_bytes(out.width, out.height) : mmhip_yuv420_frame_bytes(out.width, out.height));
    while (!max_frames || out.frames < max_frames) {
        if (!read_line(f, line, 4096)) break;
        if (line.compare(0, 5, "FRAME") != 0 || line.back() != '\n' || (line[5] != ' ' && line[5] != '\n')) {
            err = "`" + name + "': frame " + std::to_string(out.frames) + " does not begin with a FRAME line";
            return done(false);
        }
        const size_t at = out.payloads.size();
        out.payloads.resize(at + frame_bytes);
        const size_t got = fread(out.payloads.data() + at, 1, frame_bytes, f);
        if (got != frame_bytes) {
            err = "`" + name + "': frame " + std::to_string(out.frames) + " is truncated: " + std::to_string(got) + " of " + std::to_string(frame_bytes) + " bytes";
            return done(false);
        }
        ++out.frames;
    }
    if (!out.frames) { err = "`" + name + "': the stream has no frames"; return done(false); }
    return done(true);
}

// --input-frames: a define's value with exactly one %d-style conversion (%d, %04d, ...; %% is a literal percent sign)
// names one file per frame.  0: no conversion, 1: such a pattern, -1: anything else snprintf must not be handed.
int frame_pattern(const std::string &v) {
    int conversions = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (v[i] != '%') continue;
        if (i + 1 < v.size() && v[i + 1] == '%') { ++i; continue; }
        size_t j = i + 1;
        while (j < v.size() && isdigit((unsigned char)v[j])) ++j;
        if (j >= v.size() || v[j] != 'd' || j - i > 6) return -1;
        ++conversions;
        i = j;
    }
    return conversions == 0 ? 0 : conversions == 1 ? 1 : -1;
}
std::string frame_file(const std::string &pattern, int frame) {
    char name[4096];
    snprintf(name, sizeof name, pattern.c_str(), frame);
    return name;
}

}  // namespace

enum {
    OPT_VERSION = 256, OPT_HELP, OPT_HTMLDOC, OPT_BENCH_NO_OUTPUT, OPT_BENCH_ONLY_COMPILE,
    OPT_BENCH_NO_COMPILE_TIME_LIMIT, OPT_BENCH_NO_BACKEND, OPT_BENCH_RENDER_COUNT, OPT_GAUSS_MODE, OPT_INPUT_FRAMES, OPT_BATCH_FRAMES,
    OPT_NATIVE_INPUT_FRAME, OPT_SHUTTER_SAMPLES, OPT_SHUTTER, OPT_SHUTTER_MODE, OPT_AA, OPT_AA_THRESHOLD, OPT_AA_REFINE, OPT_AA_FILTER,
    OPT_YUV_MATRIX, OPT_YUV_RANGE, OPT_FPS, OPT_INPUT_YUV_MATRIX, OPT_INPUT_YUV_RANGE, OPT_INPUT_CHROMA, OPT_PIXEL_FORMAT,
    OPT_CHROMA_SITING, OPT_INPUT_CHROMA_SITING
};

int main(int argc, char **argv) {
    std::string script;
    bool have_script = false, htmldoc = false, bench_no_output = false, bench_no_backend = false;
    int antialiasing = 0, supersampling = 0, img_width = 0, img_height = 0, size_is_set = 0;
    int bench_render_count = 1, num_frames = 1, input_frames = 0, gauss_mode = MMHIP_GAUSS_EXACT, batch_frames = 1;
    int native_input_frame = MMHIP_NATIVE_FRAME_ZERO, shutter_samples = 1, aa_x = 1, aa_y = 1;
    double shutter = 0.5;
    bool shutter_fused = false, adaptive = false, aa_refine_set = false;
    float aa_threshold = 0.0f;
    int aa_refine = MMHIP_AA_REFINE_AUTO;
    bool aa_set = false, filtered = false;
    int aa_kernel = MMHIP_AA_BOX;
    float aa_radius = 0.5f;
    int yuv_matrix = MMHIP_YUV_BT709, yuv_range = MMHIP_YUV_LIMITED, fps_num = 25, fps_den = 1;      // quicktime_set_video(..., 25, ...), mathmap_cmdline.c:817-863
    bool yuv_options = false, batch_frames_set = false;
    bool pixel_format_set = false, deep = false;      // --pixel-format, and whether it is yuv420p10
    int input_yuv_matrix = MMHIP_YUV_BT709, input_yuv_range = -1, input_chroma = MMHIP_YUV_CHROMA_BILINEAR;      // -1: the stream's, else limited
    bool input_yuv_options = false, frames_set = false, fps_set = false;
    bool chroma_siting_set = false, input_chroma_siting_set = false;
    int chroma_siting = MMHIP_YUV_SITING_CENTER, input_chroma_siting = MMHIP_YUV_SITING_CENTER;      // the latter -1 for auto: the stream's tag
    const char *generator = nullptr;
    std::vector<Define> defines;
    static struct option long_options[] = {
        {"version", no_argument, 0, OPT_VERSION}, {"help", no_argument, 0, OPT_HELP},
        {"intersampling", no_argument, 0, 'i'}, {"oversampling", no_argument, 0, 'o'},
        {"cache", required_argument, 0, 'c'}, {"generator", required_argument, 0, 'g'},
        {"size", required_argument, 0, 's'}, {"script-file", required_argument, 0, 'f'},
        {"htmldoc", no_argument, 0, OPT_HTMLDOC}, {"bench-no-output", no_argument, 0, OPT_BENCH_NO_OUTPUT},
        {"bench-only-compile", no_argument, 0, OPT_BENCH_ONLY_COMPILE},
        {"bench-no-compile-time-limit", no_argument, 0, OPT_BENCH_NO_COMPILE_TIME_LIMIT},
        {"bench-no-backend", no_argument, 0, OPT_BENCH_NO_BACKEND},
        {"bench-render-count", required_argument, 0, OPT_BENCH_RENDER_COUNT},
        {"frames", required_argument, 0, 'F'}, {"gauss-mode", required_argument, 0, OPT_GAUSS_MODE},
        {"input-frames", required_argument, 0, OPT_INPUT_FRAMES}, {"batch-frames", required_argument, 0, OPT_BATCH_FRAMES},
        {"native-input-frame", required_argument, 0, OPT_NATIVE_INPUT_FRAME},
        {"shutter-samples", required_argument, 0, OPT_SHUTTER_SAMPLES}, {"shutter", required_argument, 0, OPT_SHUTTER},
        {"shutter-mode", required_argument, 0, OPT_SHUTTER_MODE}, {"aa", required_argument, 0, OPT_AA},
        {"aa-threshold", required_argument, 0, OPT_AA_THRESHOLD}, {"aa-refine", required_argument, 0, OPT_AA_REFINE},
        {"aa-filter", required_argument, 0, OPT_AA_FILTER}, {"yuv-matrix", required_argument, 0, OPT_YUV_MATRIX},
        {"yuv-range", required_argument, 0, OPT_YUV_RANGE}, {"fps", required_argument, 0, OPT_FPS},
        {"input-yuv-matrix", required_argument, 0, OPT_INPUT_YUV_MATRIX}, {"input-yuv-range", required_argument, 0, OPT_INPUT_YUV_RANGE},
        {"input-chroma", required_argument, 0, OPT_INPUT_CHROMA}, {"pixel-format", required_argument, 0, OPT_PIXEL_FORMAT},
        {"chroma-siting", required_argument, 0, OPT_CHROMA_SITING}, {"input-chroma-siting", required_argument, 0, OPT_INPUT_CHROMA_SITING},
        {0, 0, 0, 0}};
    for (;;) {
        int idx;
        int option = getopt_long(argc, argv, "f:ioF:D:c:g:s:", long_options, &idx);
        if (option == -1) break;
        switch (option) {
            case OPT_VERSION:
                printf("MathMap (HIP backend) %s\n", mmhip_version());
                return 0;
            case OPT_HELP: usage(); return 0;
            case OPT_HTMLDOC: htmldoc = true; break;
            case 'f': {
                FILE *f = fopen(optarg, "rb");
                if (!f) { fprintf(stderr, "Error: The script file `%s' could not be read.\n", optarg); return 1; }
                char buf[4096];
                size_t n;
                while ((n = fread(buf, 1, sizeof buf, f)) > 0) script.append(buf, n);
                fclose(f);
                have_script = true;
                break;
            }
            case 'i': antialiasing = 1; break;
            case 'o': supersampling = 1; break;
            case 'c': cache_size = atoi(optarg); break;
            case 'D': {
                const char *eq = strchr(optarg, '=');
                if (!eq) { fprintf(stderr, "Error: No equal sign in -D option.\n"); return 1; }
                defines.push_back({std::string(optarg, eq - optarg), std::string(eq + 1)});
                break;
            }
            case 'g': generator = optarg; break;
            case 's':
                if (sscanf(optarg, "%dx%d", &img_width, &img_height) != 2 || img_width <= 0 || img_height <= 0) {
                    fprintf(stderr, "Error: Invalid image size.  Syntax is <width>x<height>.  Example: 1024x768.\n");
                    return 1;
                }
                size_is_set = 1;
                break;
            case 'F': num_frames = atoi(optarg); if (num_frames < 1) num_frames = 1; frames_set = true; break;
            case OPT_BENCH_RENDER_COUNT: bench_render_count = atoi(optarg); break;
            case OPT_BENCH_ONLY_COMPILE: bench_render_count = 0; break;
            case OPT_BENCH_NO_OUTPUT: bench_no_output = true; break;
            case OPT_BENCH_NO_COMPILE_TIME_LIMIT: break;
            case OPT_BENCH_NO_BACKEND: bench_no_backend = true; break;
            case OPT_GAUSS_MODE:
                if (!strcmp(optarg, "exact")) gauss_mode = MMHIP_GAUSS_EXACT;
                else if (!strcmp(optarg, "tolerance")) gauss_mode = MMHIP_GAUSS_TOLERANCE;
                else { fprintf(stderr, "Error: --gauss-mode takes exact or tolerance.\n"); return 1; }
                break;
            case OPT_NATIVE_INPUT_FRAME:
                if (!strcmp(optarg, "zero")) native_input_frame = MMHIP_NATIVE_FRAME_ZERO;
                else if (!strcmp(optarg, "current")) native_input_frame = MMHIP_NATIVE_FRAME_CURRENT;
                else { fprintf(stderr, "Error: --native-input-frame takes zero or current.\n"); return 1; }
                break;
            case OPT_INPUT_FRAMES: {
                char *end = nullptr;
                long n = strtol(optarg, &end, 10);
                if (end == optarg || *end || n < 1 || n > 1000000) { fprintf(stderr, "Error: --input-frames takes a number of frames, at least 1.\n"); return 1; }
                input_frames = (int)n;
                break;
            }
            case OPT_BATCH_FRAMES: {
                char *end = nullptr;
                long n = strtol(optarg, &end, 10);
                if (end == optarg || *end || n < 1 || n > 65535) { fprintf(stderr, "Error: --batch-frames takes a number of frames, 1 to 65535.\n"); return 1; }
                batch_frames = (int)n;
                batch_frames_set = true;
                break;
            }
            case OPT_YUV_MATRIX:
                if (!strcmp(optarg, "bt601")) yuv_matrix = MMHIP_YUV_BT601;
                else if (!strcmp(optarg, "bt709")) yuv_matrix = MMHIP_YUV_BT709;
                else { fprintf(stderr, "Error: --yuv-matrix takes bt601 or bt709.\n"); return 1; }
                yuv_options = true;
                break;
            case OPT_YUV_RANGE:
                if (!strcmp(optarg, "limited")) yuv_range = MMHIP_YUV_LIMITED;
                else if (!strcmp(optarg, "full")) yuv_range = MMHIP_YUV_FULL;
                else { fprintf(stderr, "Error: --yuv-range takes limited or full.\n"); return 1; }
                yuv_options = true;
                break;
            case OPT_FPS: {
                char *end = nullptr;
                long n = strtol(optarg, &end, 10), d = 1;
                bool ok = end != optarg;
                if (ok && *end == ':') {
                    const char *second = end + 1;
                    d = strtol(second, &end, 10);
                    ok = end != second;
                }
                if (!ok || *end || n < 1 || n > 1000000000 || d < 1 || d > 1000000000) {
                    fprintf(stderr, "Error: --fps takes a frame rate N or N:D of positive integers, like 25 or 30000:1001.\n");
                    return 1;
                }
                fps_num = (int)n;
                fps_den = (int)d;
                yuv_options = true;
                fps_set = true;
                break;
            }
            case OPT_PIXEL_FORMAT:
                if (!strcmp(optarg, "yuv420p")) deep = false;
                else if (!strcmp(optarg, "yuv420p10")) deep = true;
                else { fprintf(stderr, "Error: --pixel-format takes yuv420p or yuv420p10.\n"); return 1; }
                pixel_format_set = true;
                break;
            case OPT_CHROMA_SITING:
                if (!strcmp(optarg, "center")) chroma_siting = MMHIP_YUV_SITING_CENTER;
                else if (!strcmp(optarg, "left")) chroma_siting = MMHIP_YUV_SITING_LEFT;
                else { fprintf(stderr, "Error: --chroma-siting takes center or left.\n"); return 1; }
                chroma_siting_set = true;
                break;
            case OPT_INPUT_CHROMA_SITING:
                if (!strcmp(optarg, "center")) input_chroma_siting = MMHIP_YUV_SITING_CENTER;
                else if (!strcmp(optarg, "left")) input_chroma_siting = MMHIP_YUV_SITING_LEFT;
                else if (!strcmp(optarg, "auto")) input_chroma_siting = -1;
                else { fprintf(stderr, "Error: --input-chroma-siting takes center, left or auto.\n"); return 1; }
                input_chroma_siting_set = true;
                break;
            case OPT_INPUT_YUV_MATRIX:
                if (!strcmp(optarg, "bt601")) input_yuv_matrix = MMHIP_YUV_BT601;
                else if (!strcmp(optarg, "bt709")) input_yuv_matrix = MMHIP_YUV_BT709;
                else { fprintf(stderr, "Error: --input-yuv-matrix takes bt601 or bt709.\n"); return 1; }
                input_yuv_options = true;
                break;
            case OPT_INPUT_YUV_RANGE:
                if (!strcmp(optarg, "limited")) input_yuv_range = MMHIP_YUV_LIMITED;
                else if (!strcmp(optarg, "full")) input_yuv_range = MMHIP_YUV_FULL;
                else { fprintf(stderr, "Error: --input-yuv-range takes limited or full.\n"); return 1; }
                input_yuv_options = true;
                break;
            case OPT_INPUT_CHROMA:
                if (!strcmp(optarg, "bilinear")) input_chroma = MMHIP_YUV_CHROMA_BILINEAR;
                else if (!strcmp(optarg, "replicate")) input_chroma = MMHIP_YUV_CHROMA_REPLICATE;
                else { fprintf(stderr, "Error: --input-chroma takes bilinear or replicate.\n"); return 1; }
                input_yuv_options = true;
                break;
            case OPT_SHUTTER_SAMPLES: {
                char *end = nullptr;
                long n = strtol(optarg, &end, 10);
                if (end == optarg || *end || n < 1 || n > MMHIP_SHUTTER_MAX_SAMPLES) { fprintf(stderr, "Error: --shutter-samples takes a number of samples, 1 to %d.\n", (int)MMHIP_SHUTTER_MAX_SAMPLES); return 1; }
                shutter_samples = (int)n;
                break;
            }
            case OPT_SHUTTER_MODE:
                if (!strcmp(optarg, "maps")) shutter_fused = false;
                else if (!strcmp(optarg, "fused")) shutter_fused = true;
                else { fprintf(stderr, "Error: --shutter-mode takes maps or fused.\n"); return 1; }
                break;
            case OPT_AA: {
                char *end = nullptr;
                long nx = strtol(optarg, &end, 10), ny = nx;
                bool ok = end != optarg;
                if (ok && *end == 'x') {
                    const char *second = end + 1;
                    ny = strtol(second, &end, 10);
                    ok = end != second;
                }
                if (!ok || *end || nx < 1 || nx > MMHIP_SAMPLE_GRID_MAX || ny < 1 || ny > MMHIP_SAMPLE_GRID_MAX) {
                    fprintf(stderr, "Error: --aa takes N or SXxSY, 1 to %d each.\n", (int)MMHIP_SAMPLE_GRID_MAX);
                    return 1;
                }
                aa_x = (int)nx;
                aa_y = (int)ny;
                aa_set = true;
                break;
            }
            case OPT_AA_FILTER: {
                static const struct { const char *name; int kernel; float radius; } kernels[] = {
                    {"box", MMHIP_AA_BOX, 0.5f}, {"tent", MMHIP_AA_TENT, 1.0f}, {"gaussian", MMHIP_AA_GAUSSIAN, 1.5f}, {"mitchell", MMHIP_AA_MITCHELL, 2.0f}};
                const char *colon = strchr(optarg, ':');
                const std::string name = colon ? std::string(optarg, colon - optarg) : std::string(optarg);
                bool ok = false;
                for (const auto &k : kernels)
                    if (name == k.name) {
                        aa_kernel = k.kernel;
                        aa_radius = k.radius;
                        ok = true;
                    }
                if (ok && colon) {
                    char *end = nullptr;
                    aa_radius = strtof(colon + 1, &end);
                    ok = end != colon + 1 && !*end && std::isfinite(aa_radius) && aa_radius >= 0.5f && aa_radius <= 4.0f;
                }
                if (!ok) {
                    fprintf(stderr, "Error: --aa-filter takes box, tent, gaussian or mitchell, and behind a colon a radius from 0.5 to 4.\n");
                    return 1;
                }
                filtered = true;
                break;
            }
            case OPT_AA_THRESHOLD: {
                char *end = nullptr;
                aa_threshold = strtof(optarg, &end);
                if (end == optarg || *end || std::isnan(aa_threshold)) { fprintf(stderr, "Error: --aa-threshold takes a number, like 0.05.\n"); return 1; }
                adaptive = true;
                break;
            }
            case OPT_AA_REFINE:
                if (!strcmp(optarg, "list")) aa_refine = MMHIP_AA_REFINE_AUTO;
                else if (!strcmp(optarg, "select")) aa_refine = MMHIP_AA_REFINE_SELECT;
                else { fprintf(stderr, "Error: --aa-refine takes list or select.\n"); return 1; }
                aa_refine_set = true;
                break;
            case OPT_SHUTTER: {
                char *end = nullptr;
                shutter = strtod(optarg, &end);
                if (end == optarg || *end || !std::isfinite(shutter)) { fprintf(stderr, "Error: --shutter takes a fraction of the frame interval, like 0.5.\n"); return 1; }
                break;
            }
            default: usage(); return 1;
        }
    }
    if (aa_refine_set && !adaptive) {
        fprintf(stderr, "Error: --aa-refine goes with --aa-threshold.\n");
        return 1;
    }
    if (adaptive && supersampling) {
        fprintf(stderr, "Error: --aa-threshold is not combined with -o (oversampling).\n");
        return 1;
    }
    if (adaptive && shutter_samples > 1) {
        fprintf(stderr, "Error: --aa-threshold is not combined with --shutter-samples.\n");
        return 1;
    }
    if (adaptive && aa_x * aa_y == 1) {
        fprintf(stderr, "Error: --aa-threshold goes with --aa.\n");
        return 1;
    }
    if (filtered && !aa_set) {
        fprintf(stderr, "Error: --aa-filter goes with --aa (which may be --aa=1).\n");
        return 1;
    }
    if (filtered && supersampling) {
        fprintf(stderr, "Error: --aa-filter is not combined with -o (oversampling).\n");
        return 1;
    }
    if (filtered && adaptive) {
        fprintf(stderr, "Error: --aa-filter is not combined with --aa-threshold.\n");
        return 1;
    }
    if (filtered && shutter_fused) {
        fprintf(stderr, "Error: --aa-filter is not combined with --shutter-mode=fused.\n");
        return 1;
    }
    if (supersampling && shutter_samples > 1) {
        fprintf(stderr, "Error: --shutter-samples is not combined with -o (oversampling).\n");
        return 1;
    }
    const bool sampled = aa_x * aa_y > 1;
    if (supersampling && sampled) {
        fprintf(stderr, "Error: --aa is not combined with -o (oversampling).\n");
        return 1;
    }
    if (shutter_samples * aa_x * aa_y > MMHIP_SHUTTER_MAX_SAMPLES) {
        fprintf(stderr, "Error: --shutter-samples times the --aa grid is at most %d sub-samples.\n", (int)MMHIP_SHUTTER_MAX_SAMPLES);
        return 1;
    }
    const char *output_filename;
    if (have_script) {
        if (argc - optind != 1) { usage(); return 1; }
        output_filename = argv[optind];
    } else {
        if (argc - optind != 2) { usage(); return 1; }
        script = argv[optind];
        output_filename = argv[optind + 1];
    }
    // an output name ending in .y4m, or - for standard output: all frames as one YUV4MPEG2 stream
    const size_t name_len = strlen(output_filename);
    const bool to_stdout = !strcmp(output_filename, "-");
    const bool y4m = to_stdout || (name_len >= 4 && !strcmp(output_filename + name_len - 4, ".y4m"));
    if (yuv_options && !y4m) {
        fprintf(stderr, "Error: --yuv-matrix, --yuv-range and --fps go with an output file name ending in .y4m (or -).\n");
        return 1;
    }
    if (chroma_siting_set && !y4m) {
        fprintf(stderr, "Error: --chroma-siting goes with an output file name ending in .y4m (or -).\n");
        return 1;
    }
    if (pixel_format_set && !y4m) {
        fprintf(stderr, "Error: --pixel-format goes with an output file name ending in .y4m (or -).\n");
        return 1;
    }
    if (deep && supersampling) {
        fprintf(stderr, "Error: --pixel-format=yuv420p10 is not combined with -o: supersampled frames are bytes.\n");
        return 1;
    }
    if (htmldoc) { fprintf(stderr, "Error: --htmldoc is not supported by the HIP command line.\n"); return 1; }
    if (generator) { fprintf(stderr, "Unknown generator `%s'\n", generator); return 1; }
    // the file of frame `frame` of an image define: the name itself unless --input-frames makes it a pattern
    auto is_pattern = [&](const Define &d) { return input_frames && frame_pattern(d.value) == 1; };
    auto sequence_of = [&](const Define &d) { return is_pattern(d) ? input_frames : 1; };
    auto file_of = [&](const Define &d, int frame) { return is_pattern(d) ? frame_file(d.value, frame) : d.value; };

    mmhip_options opts;
    mmhip_default_options(&opts);
    opts.intersample = antialiasing;
    opts.supersampling = supersampling;
    opts.gauss_mode = gauss_mode;
    // an extension next to the reference's options: a script whose first character is '{' (which no .mm text can
    // start with) is a compiled filter in the IR dump form of mmhip_filter_ir_json_raw, e.g. the output of another
    // front-end; everything after compilation is the same
    size_t first = script.find_first_not_of(" \t\r\n");
    const bool is_ir = first != std::string::npos && script[first] == '{';
    mmhip_filter *flt = is_ir ? mmhip_compile_ir_json(script.c_str(), &opts) : mmhip_compile(script.c_str(), &opts);
    if (bench_no_backend) return 0;
    if (!flt) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
    if (bench_render_count == 0) return mmhip_filter_jit(flt, 0) < 0 ? 1 : 0;

    auto lookup = [&](const char *name) -> const Define * {
        for (const Define &d : defines) if (d.name == name) return &d;
        return nullptr;
    };
    int nuv = mmhip_filter_num_uservals(flt);
    for (int i = 0; i < nuv && input_frames; ++i) {      // (the defines of image user values only: other values may hold a '%')
        mmhip_userval_info info;
        mmhip_filter_userval_info(flt, i, &info);
        const Define *d = info.kind == MMHIP_UV_IMAGE ? lookup(info.name) : nullptr;
        if (d && frame_pattern(d->value) < 0) {
            fprintf(stderr, "Error: `%s': with --input-frames an image file name takes one conversion like %%d or %%04d.\n", d->value.c_str());
            return 1;
        }
    }
    // image defines that name a YUV4MPEG2 stream (a name ending in .y4m, or - for standard input): read whole, or up to
    // --input-frames frames, before the size and the number of frames are settled, which the first of them may give
    std::vector<Y4mStream> streams;
    int from_stdin = 0;
    for (int i = 0; i < nuv; ++i) {
        mmhip_userval_info info;
        mmhip_filter_userval_info(flt, i, &info);
        const Define *d = info.kind == MMHIP_UV_IMAGE ? lookup(info.name) : nullptr;
        if (!d || !is_y4m_name(d->value)) continue;
        from_stdin += d->value == "-";
        streams.emplace_back();
        streams.back().uv = i;
    }
    if (input_chroma_siting_set && streams.empty()) {
        fprintf(stderr, "Error: --input-chroma-siting goes with an input image whose file name ends in .y4m (or is -).\n");
        return 1;
    }
    if (input_yuv_options && streams.empty()) {
        fprintf(stderr, "Error: --input-yuv-matrix, --input-yuv-range and --input-chroma go with an input image whose file name ends in .y4m (or is -).\n");
        return 1;
    }
    if (from_stdin > 1) {
        fprintf(stderr, "Error: At most one input image can be read from standard input (-).\n");
        return 1;
    }
    for (Y4mStream &st : streams) {
        mmhip_userval_info info;
        mmhip_filter_userval_info(flt, st.uv, &info);
        std::string err;
        if (!read_y4m(lookup(info.name)->value, input_frames, st, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    }
    // a 10-bit stream is bound as a float32 drawable: the filter is compiled once more, for such inputs (its user values
    // are the same)
    bool deep_input = false;
    for (const Y4mStream &st : streams) deep_input = deep_input || st.bits == 10;
    if (deep_input) {
        mmhip_filter_free(flt);
        opts.deep_inputs = 1;
        flt = is_ir ? mmhip_compile_ir_json(script.c_str(), &opts) : mmhip_compile(script.c_str(), &opts);
        if (!flt) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
    }
    auto stream_of = [&](int uv) -> const Y4mStream * {
        for (const Y4mStream &st : streams) if (st.uv == uv) return &st;
        return nullptr;
    };
    if (!streams.empty()) {
        if (!frames_set) num_frames = streams[0].frames;
        if (y4m && !fps_set) { fps_num = streams[0].fps_num; fps_den = streams[0].fps_den; }
    }
    std::vector<unsigned char> pixels;
    if (!size_is_set)
        for (int i = 0; i < nuv; ++i) {
            mmhip_userval_info info;
            mmhip_filter_userval_info(flt, i, &info);
            if (info.kind != MMHIP_UV_IMAGE) continue;
            const Define *d = lookup(info.name);
            if (!d) { fprintf(stderr, "Error: No value defined for input image `%s'.\n", info.name); return 1; }
            if (const Y4mStream *st = stream_of(i)) {
                img_width = st->width;
                img_height = st->height;
                size_is_set = 1;
                break;
            }
            if (!read_png(file_of(*d, 0).c_str(), pixels, img_width, img_height)) {
                fprintf(stderr, "Error: Could not read input image `%s'.\n", file_of(*d, 0).c_str());
                return 1;
            }
            size_is_set = 1;
            break;
        }
    if (!size_is_set) { fprintf(stderr, "Error: Image size not set and no input images given.\n"); return 1; }

    mmhip_invocation *inv = mmhip_invoke(flt, img_width, img_height);
    if (!inv) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
    if (mmhip_set_native_input_frame(inv, native_input_frame) != 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
    for (int i = 0; i < nuv; ++i) {
        mmhip_userval_info info;
        mmhip_filter_userval_info(flt, i, &info);
        const Define *d = lookup(info.name);
        if (!d) {
            if (info.kind == MMHIP_UV_IMAGE) { fprintf(stderr, "Error: No value defined for input image `%s'.\n", info.name); return 1; }
            continue;
        }
        switch (info.kind) {
            case MMHIP_UV_INT: mmhip_set_int(inv, i, atoi(d->value.c_str())); break;
            case MMHIP_UV_FLOAT: mmhip_set_float(inv, i, (float)strtod(d->value.c_str(), nullptr)); break;
            case MMHIP_UV_BOOL: mmhip_set_bool(inv, i, (int)(float)atoi(d->value.c_str())); break;
            case MMHIP_UV_IMAGE: {
                if (const Y4mStream *st = stream_of(i)) {
                    const int range = input_yuv_range >= 0 ? input_yuv_range : st->range >= 0 ? st->range : MMHIP_YUV_LIMITED;
                    // --input-chroma-siting: left, or auto on a stream tagged C420mpeg2, takes the _sited setters; centre is the call below
                    const int siting = input_chroma_siting >= 0 ? input_chroma_siting : st->siting;
                    if (siting != MMHIP_YUV_SITING_CENTER) {
                        const int rc = st->bits == 10
                                           ? mmhip_set_image_sequence_yuv420p10_host_sited(inv, i, (const uint16_t *)st->payloads.data(),
                                                                                           mmhip_yuv420p10_frame_bytes(st->width, st->height), st->width,
                                                                                           st->height, st->frames, input_yuv_matrix, range, input_chroma, siting)
                                           : mmhip_set_image_sequence_yuv420_host_sited(inv, i, st->payloads.data(),
                                                                                        mmhip_yuv420_frame_bytes(st->width, st->height), st->width,
                                                                                        st->height, st->frames, input_yuv_matrix, range, input_chroma, siting);
                        if (rc != 0) {
                            fprintf(stderr, "Error: %s\n", mmhip_last_error());
                            return 1;
                        }
                        break;
                    }
                    if (st->bits == 10) {
                        // (the bytes of a file are little-endian samples, which is this host's order)
                        if (mmhip_set_image_sequence_yuv420p10_host(inv, i, (const uint16_t *)st->payloads.data(),
                                                                    mmhip_yuv420p10_frame_bytes(st->width, st->height), st->width, st->height, st->frames,
                                                                    input_yuv_matrix, range, input_chroma) != 0) {
                            fprintf(stderr, "Error: %s\n", mmhip_last_error());
                            return 1;
                        }
                        break;
                    }
                    if (mmhip_set_image_sequence_yuv420_host(inv, i, st->payloads.data(), mmhip_yuv420_frame_bytes(st->width, st->height), st->width,
                                                             st->height, st->frames, input_yuv_matrix, range, input_chroma) != 0) {
                        fprintf(stderr, "Error: %s\n", mmhip_last_error());
                        return 1;
                    }
                    break;
                }
                // one file, or with --input-frames and a %d in the name one file per frame, all of one size
                const int n = sequence_of(*d);
                std::vector<unsigned char> frames;
                int w = 0, h = 0;
                for (int k = 0; k < n; ++k) {
                    const std::string file = file_of(*d, k);
                    int fw, fh;
                    if (!read_png(file.c_str(), pixels, fw, fh)) {
                        fprintf(stderr, "Error: Could not read input image `%s'.\n", file.c_str());
                        return 1;
                    }
                    if (k > 0 && (fw != w || fh != h)) {
                        fprintf(stderr, "Error: Input image `%s' is %dx%d, but frame 0 of `%s' is %dx%d: all frames of an input must have one size.\n",
                                file.c_str(), fw, fh, info.name, w, h);
                        return 1;
                    }
                    w = fw; h = fh;
                    frames.insert(frames.end(), pixels.begin(), pixels.begin() + (size_t)w * h * 3);
                }
                if (mmhip_set_image_sequence_host(inv, i, frames.data(), w, h, 3, n) != 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
                break;
            }
            default:
                fprintf(stderr, "Error: Can only define user values for types int, float, bool and image.\n");
                return 1;
        }
    }

    std::vector<unsigned char> output((size_t)img_width * img_height * 4);
    auto write_frame = [&](int frame) {
        char name[4096];
        if (num_frames > 1 && strstr(output_filename, "%")) snprintf(name, sizeof name, output_filename, frame);
        else snprintf(name, sizeof name, "%s", output_filename);
        if (!write_png_rgb(name, output.data(), img_width, img_height)) {
            fprintf(stderr, "Error: Cannot open file `%s' for writing: %s\n", name, strerror(errno));
            return false;
        }
        return true;
    };
    // --batch-frames=K: K frames per clip render (one batched launch where the filter allows it), then the files one by
    // one; a batch's frames stay under 1 GiB of device memory.  With -o the clip is a supersampled one.
    // --shutter-samples=K: the frames go through mmhip_render_clip_shutter (--shutter-mode=fused: ..._fused), --batch-frames of them per call (by default
    // one, all of its K sub-samples in one nested clip), at the span (float)((double)FRACTION / NUM).
    // --aa: they go through mmhip_render_clip_sampled (..._fused) instead, with or without a shutter.
    // --aa-threshold: through mmhip_render_clip_adaptive.  --aa-filter: through mmhip_render_clip_filtered.
    const bool shuttered = shutter_samples > 1 || sampled || filtered;
    const float shutter_span = (float)(shutter / (double)num_frames);
    // A .y4m output: every batch is converted to planar 4:2:0 on the device (mmhip_clip_to_yuv420), its payloads come
    // over in one copy, and each goes to the file behind "FRAME\n".  Without --batch-frames a batch is what fits in the
    // 1 GiB of RGBA8 staging.
    if (y4m && !batch_frames_set) batch_frames = 65535;
    // --pixel-format=yuv420p10: the batches land as float maps, 16 bytes per pixel, and mmhip_clip_float_to_yuv420p10
    // converts those.
    const size_t landed_frame = deep ? output.size() * 4 : output.size();
    const int landed_floatmap = deep ? 1 : 0;
    batch_frames = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(batch_frames, num_frames), ((size_t)1 << 30) / landed_frame));
    void *dev = mmhip_device_alloc(landed_frame * batch_frames);
    if (!dev) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
    const size_t yuv_frame = !y4m ? 0 : (size_t)(deep ? mmhip_yuv420p10_frame_bytes(img_width, img_height) : mmhip_yuv420_frame_bytes(img_width, img_height));
    void *yuv_dev = nullptr;
    std::vector<unsigned char> yuv_host;
    FILE *movie = nullptr;
    if (y4m) {
        yuv_dev = mmhip_device_alloc(yuv_frame * batch_frames);
        if (!yuv_dev) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
        yuv_host.resize(yuv_frame * batch_frames);
        char header[160];
        const bool left = chroma_siting == MMHIP_YUV_SITING_LEFT;      // (an 8-bit stream is then tagged C420mpeg2)
        const int header_len = left ? mmhip_y4m_header_sited(header, sizeof header, img_width, img_height, fps_num, fps_den, yuv_range, deep ? 10 : 8, chroma_siting)
                                    : (deep ? mmhip_y4m_header_p10 : mmhip_y4m_header)(header, sizeof header, img_width, img_height, fps_num, fps_den, yuv_range);
        if (header_len < 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
        if (!bench_no_output) {
            movie = to_stdout ? stdout : fopen(output_filename, "wb");
            if (!movie || fwrite(header, 1, (size_t)header_len, movie) != (size_t)header_len) {
                fprintf(stderr, "Error: Cannot open file `%s' for writing: %s\n", output_filename, strerror(errno));
                return 1;
            }
        }
    }
    const bool left_sited = y4m && chroma_siting == MMHIP_YUV_SITING_LEFT;      // --chroma-siting=left: the _sited converters
    for (int render_num = 0; render_num < bench_render_count; ++render_num) {
        const bool last_render = render_num == bench_render_count - 1;      // (the movie holds the frames once)
        for (int first = 0; (batch_frames > 1 || shuttered || y4m) && first < num_frames; first += batch_frames) {
            const int n = std::min(batch_frames, num_frames - first);
            std::vector<int> frames(n);
            std::vector<float> ts(n);
            for (int i = 0; i < n; ++i) {
                frames[i] = first + i;
                ts[i] = (float)(first + i) / (float)num_frames;       // mathmap_cmdline.c:835
            }
            const int rc = filtered
                               ? mmhip_render_clip_filtered(inv, n, frames.data(), ts.data(), shutter_samples, shutter_span, aa_x, aa_y, aa_kernel,
                                                            aa_radius, 0, 0, img_width, img_height, 0, img_height, dev, img_width * 4,
                                                            (int64_t)landed_frame, 4, landed_floatmap, nullptr)
                           : adaptive
                               ? mmhip_render_clip_adaptive(inv, n, frames.data(), ts.data(), aa_x, aa_y, aa_threshold, aa_refine, 0, 0, img_width,
                                                            img_height, 0, img_height, dev, img_width * 4, (int64_t)landed_frame, 4, landed_floatmap, nullptr)
                           : sampled
                               ? (shutter_fused ? mmhip_render_clip_sampled_fused : mmhip_render_clip_sampled)(
                                     inv, n, frames.data(), ts.data(), shutter_samples, shutter_span, aa_x, aa_y, 0, 0, img_width, img_height, 0,
                                     img_height, dev, img_width * 4, (int64_t)landed_frame, 4, landed_floatmap, nullptr)
                           : shuttered
                               ? (shutter_fused ? mmhip_render_clip_shutter_fused : mmhip_render_clip_shutter)(
                                     inv, n, frames.data(), ts.data(), shutter_samples, shutter_span, 0, 0, img_width, img_height, 0, img_height,
                                     dev, img_width * 4, (int64_t)landed_frame, 4, landed_floatmap, nullptr)
                           : supersampling
                               ? mmhip_render_clip_supersampled(inv, n, frames.data(), ts.data(), 0, 0, img_width, img_height, dev,
                                                                img_width * 4, (int64_t)output.size(), 4, nullptr)
                               : mmhip_render_clip(inv, n, frames.data(), ts.data(), 0, 0, img_width, img_height, 0, img_height, dev,
                                                   img_width * 4, (int64_t)landed_frame, 4, landed_floatmap, nullptr);
            if (rc != 0 ||
                (y4m && !deep && !left_sited &&
                 mmhip_clip_to_yuv420(inv, dev, (int64_t)img_width * 4, (int64_t)output.size(), img_width, img_height, 0, img_height, n, yuv_matrix,
                                      yuv_range, yuv_dev, (int64_t)yuv_frame, nullptr) != 0) ||
                (deep && !left_sited &&
                 mmhip_clip_float_to_yuv420p10(inv, dev, (int64_t)img_width * 16, (int64_t)landed_frame, img_width, img_height, 0, img_height, n, yuv_matrix,
                                               yuv_range, yuv_dev, (int64_t)yuv_frame, nullptr) != 0) ||
                (y4m && !deep && left_sited &&
                 mmhip_clip_to_yuv420_sited(inv, dev, (int64_t)img_width * 4, (int64_t)output.size(), img_width, img_height, 0, img_height, n, yuv_matrix,
                                            yuv_range, chroma_siting, yuv_dev, (int64_t)yuv_frame, nullptr) != 0) ||
                (deep && left_sited &&
                 mmhip_clip_float_to_yuv420p10_sited(inv, dev, (int64_t)img_width * 16, (int64_t)landed_frame, img_width, img_height, 0, img_height, n,
                                                     yuv_matrix, yuv_range, chroma_siting, yuv_dev, (int64_t)yuv_frame, nullptr) != 0) ||
                mmhip_sync(inv) != 0) {
                fprintf(stderr, "Error: %s\n", mmhip_last_error());
                return 1;
            }
            if (y4m) {
                if (!movie || !last_render) continue;
                if (mmhip_copy_to_host(yuv_host.data(), yuv_dev, yuv_frame * n) != 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
                for (int i = 0; i < n; ++i)
                    if (fwrite("FRAME\n", 1, 6, movie) != 6 || fwrite(yuv_host.data() + (size_t)i * yuv_frame, 1, yuv_frame, movie) != yuv_frame) {
                        fprintf(stderr, "Error: Cannot write to file `%s': %s\n", output_filename, strerror(errno));
                        return 1;
                    }
                continue;
            }
            for (int i = 0; i < n && !bench_no_output; ++i) {
                if (mmhip_copy_to_host(output.data(), (char *)dev + (size_t)i * output.size(), output.size()) != 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
                if (!write_frame(first + i)) return 1;
            }
        }
        for (int frame = 0; batch_frames == 1 && !shuttered && !y4m && frame < num_frames; ++frame) {
            float t = (float)frame / (float)num_frames;       // mathmap_cmdline.c:835
            int rc = supersampling
                         ? mmhip_render_supersampled(inv, frame, t, 0, 0, img_width, img_height, dev, img_width * 4, 4, nullptr)
                         : mmhip_render(inv, frame, t, 0, 0, img_width, img_height, 0, img_height, dev, img_width * 4, 4, 0, nullptr);
            if (rc != 0 || mmhip_sync(inv) != 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
            if (bench_no_output) continue;
            if (mmhip_copy_to_host(output.data(), dev, output.size()) != 0) { fprintf(stderr, "Error: %s\n", mmhip_last_error()); return 1; }
            if (!write_frame(frame)) return 1;
        }
    }
    if (movie && (to_stdout ? fflush(movie) : fclose(movie)) != 0) {
        fprintf(stderr, "Error: Cannot write to file `%s': %s\n", output_filename, strerror(errno));
        return 1;
    }
    mmhip_device_free(yuv_dev);
    mmhip_device_free(dev);
    mmhip_invocation_free(inv);
    mmhip_filter_free(flt);
    return 0;
}
