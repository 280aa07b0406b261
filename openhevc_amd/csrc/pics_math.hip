/*
 * pics_math.hip — the host arithmetic of the picture services (engine_pics.hip), with neither an engine nor a device: image sizes and
 * crop windows, the ids of a call (destinations apart from sources, neighbours in time), the integers of the RGB conversions, the colour tables of the HDR forms, light-level bins and percentiles, the SSIM window
 * and PSNR, the resize taps, the compose formulas, the reformat quantisation, the orientations' group, the pic_struct table, the adaptive deinterlacer's sample, the filters' taps and samples, and what follows from a histogram's bins with the table builders, the motion helpers, the warp's positions, taps and map builders, the film grain's hash, patterns, tables and samples, the colour remapping's curves, samples and per-plane tables, and the frame packing's descriptor, view sizes and samples.  No kernel, no HIP runtime call: tests/pics_math_check.cpp runs it under sanitizers.
 */
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>
#include "pics_math.h"
#include "kernels.h"
#include "compare_common.h"
#include "compose_common.h"
#include "reformat_common.h"
#include "deinterlace_common.h"
#include "filter_common.h"
#include "motion_common.h"
#include "warp_common.h"
#include "grain_common.h"
#include "remap_common.h"
#include "packing_common.h"
#include "../../include/ohevc_annexb.h"

static bool depth_ok(int bit_depth) { return bit_depth == 8 || bit_depth == 9 || bit_depth == 10 || bit_depth == 12; }

/* what a window leaves of a picture, luma samples */
void window_size(const OhPicParams *p, const OhWindow &w, int *W, int *H)
{
    *W = p->width - w.left - w.right;
    *H = p->height - w.top - w.bottom;
}

/* the window in the planes of class q (0 luma, 1 chroma): its origin in the plane and what it leaves, plane samples */
void class_window(const OhPicParams *p, const OhWindow &w, int q, int32_t *x0, int32_t *y0, int32_t *ws, int32_t *hs)
{
    const int sx = oh_hshift(p, q), sy = oh_vshift(p, q);
    int W, H;
    window_size(p, w, &W, &H);
    *x0 = w.left >> sx; *y0 = w.top >> sy;
    *ws = W >> sx; *hs = H >> sy;
}

/* a crop window of a picture: offsets not negative, something left and — aligned — the offsets multiples of the chroma sub-sampling.
 * false: *why says what is wrong. */
bool crop_window_ok(const OhPicParams *p, const OhWindow &w, bool aligned, std::string *why)
{
    const int cf = p->chroma_format_idc, sw = aligned && (cf == 1 || cf == 2) ? 2 : 1, sh = aligned && cf == 1 ? 2 : 1;
    int W, H;
    window_size(p, w, &W, &H);
    if (w.left >= 0 && w.right >= 0 && w.top >= 0 && w.bottom >= 0 && W > 0 && H > 0 && !(w.left % sw) && !(w.right % sw) && !(w.top % sh) && !(w.bottom % sh))
        return true;
    char buf[256];
    if (aligned)
        snprintf(buf, sizeof(buf), "window (%d,%d,%d,%d) of %dx%d: empty, or offsets not multiples of %dx%d", w.left, w.right, w.top, w.bottom,
                 p->width, p->height, sw, sh);
    else
        snprintf(buf, sizeof(buf), "window (%d,%d,%d,%d) leaves nothing of %dx%d", w.left, w.right, w.top, w.bottom, p->width, p->height);
    *why = buf;
    return false;
}

/* the ids of a call that writes pictures.  0: no destination is listed twice and none is among the sources; 1: one is listed twice;
 * 2: *both, the first such source, is also a destination */
int ids_apart(const int *dst_ids, int nd, const int *src_ids, int ns, int *both)
{
    std::vector<int> d(dst_ids, dst_ids + nd);
    std::sort(d.begin(), d.end());
    if (std::adjacent_find(d.begin(), d.end()) != d.end())
        return 1;
    for (int i = 0; i < ns; i++)
        if (std::binary_search(d.begin(), d.end(), src_ids[i])) {
            *both = src_ids[i];
            return 2;
        }
    return 0;
}

/* the pictures before (around[0]) and after (around[1]) each of the n pictures own_ids in time: around_ids[k][i], where a null array
 * or an entry of -1 stands for the picture itself; *srcs: own_ids, then the lists that were given.  Not used (the mode does not read
 * them): the arrays are not read and every picture stands for itself.  -1: done; else the index of the first entry below -1, in
 * list *side */
int neighbours_resolve(const int *const around_ids[2], const int *own_ids, int n, bool used, std::vector<int> around[2],
                       std::vector<int> *srcs, int *side)
{
    srcs->assign(own_ids, own_ids + n);
    for (int k = 0; k < 2; k++) {
        const int *ids = around_ids[k];
        around[k].assign(own_ids, own_ids + n);
        if (!used || !ids)
            continue;
        for (int i = 0; i < n; i++) {
            if (ids[i] < -1) {
                *side = k;
                return i;
            }
            if (ids[i] >= 0)
                around[k][i] = ids[i];
        }
        srcs->insert(srcs->end(), around[k].begin(), around[k].end());
    }
    return -1;
}

/* ---------------- conversion to standard images (convert.hip) ---------------- */
int conv_sample_bytes(const OhConvert *cv, int bit_depth)
{
    switch (cv->sample) {
    case OH_CONV_NATIVE: return bit_depth > 8 ? 2 : 1;
    case OH_CONV_U8:     return 1;
    case OH_CONV_F32:    return 4;
    default:             return 2;
    }
}

/* what oh_pics_convert checks of the combination itself (not of pictures or memory); *bytes: one image */
int conv_check(const OhPicParams *p, const OhConvert *cv, size_t *bytes, std::string *why)
{
    char buf[256];
    if (!p || !cv) { *why = "no params or no OhConvert"; return OH_E_ARG; }
    const int cf = p->chroma_format_idc, bd = p->bit_depth;
    if (p->width <= 0 || p->height <= 0 || cf < 0 || cf > 3 || !depth_ok(bd)) {
        *why = "bad picture params"; return OH_E_ARG;
    }
    if (cv->format < OH_CONV_PLANAR || cv->format > OH_CONV_RGBA || cv->sample < OH_CONV_NATIVE || cv->sample > OH_CONV_F32) {
        snprintf(buf, sizeof(buf), "format %d / sample %d unknown", cv->format, cv->sample); *why = buf; return OH_E_UNSUPPORTED;
    }
    const bool yuv = cv->format <= OH_CONV_SEMIPLANAR;
    if (yuv ? cv->sample > OH_CONV_U8 : cv->sample == OH_CONV_NATIVE) {
        snprintf(buf, sizeof(buf), "sample %d does not fit format %d (YUV: NATIVE or U8; RGB: U8, U16, F16, F32)", cv->sample, cv->format);
        *why = buf; return OH_E_UNSUPPORTED;
    }
    if (!yuv && cv->matrix != 1 && cv->matrix != 5 && cv->matrix != 6 && cv->matrix != 9) {
        snprintf(buf, sizeof(buf), "matrix_coefficients %d (1 BT.709, 5 / 6 BT.601, 9 BT.2020 NCL)", cv->matrix); *why = buf; return OH_E_UNSUPPORTED;
    }
    if (cv->format == OH_CONV_SEMIPLANAR && cf == 0) { *why = "a 4:0:0 picture has no semi-planar form"; return OH_E_UNSUPPORTED; }
    if ((cv->full_range != 0 && cv->full_range != 1) || (cv->chroma_filter != 0 && cv->chroma_filter != 1)) {
        *why = "full_range and chroma_filter are 0 or 1"; return OH_E_ARG;
    }
    if (!crop_window_ok(p, cv->win, true, why))
        return OH_E_ARG;
    const int sw = (cf == 1 || cf == 2) ? 2 : 1, sh = cf == 1 ? 2 : 1;
    int W, H;
    window_size(p, cv->win, &W, &H);
    size_t samples;
    if (cv->format <= OH_CONV_SEMIPLANAR)
        samples = (size_t)W * H + (cf ? 2 * (size_t)(W / sw) * (H / sh) : 0);
    else
        samples = (size_t)W * H * (cv->format == OH_CONV_RGBA ? 4 : 3);
    *bytes = samples * (size_t)conv_sample_bytes(cv, bd);
    return OH_OK;
}

extern "C" size_t oh_convert_image_bytes(const OhPicParams *p, const OhConvert *cv)
{
    size_t bytes = 0;
    std::string why;
    return conv_check(p, cv, &bytes, &why) == OH_OK ? bytes : 0;
}

/* what both coefficient functions refuse (n_min: the entries `out` must have), and kr and kb of the matrix_coefficients code */
static int coeffs_check(const OhConvert *cv, int bit_depth, const int32_t *out, int n, int n_min, double *kr, double *kb)
{
    if (!cv || !out || n < n_min || !depth_ok(bit_depth))
        return OH_E_ARG;
    if (cv->format < OH_CONV_RGB_PLANAR || cv->format > OH_CONV_RGBA || cv->sample < OH_CONV_U8 || cv->sample > OH_CONV_F32)
        return OH_E_UNSUPPORTED;
    switch (cv->matrix) {
    case 1:  *kr = 0.2126; *kb = 0.0722; break;
    case 5:
    case 6:  *kr = 0.299;  *kb = 0.114;  break;
    case 9:  *kr = 0.2627; *kb = 0.0593; break;
    default: return OH_E_UNSUPPORTED;
    }
    return cv->full_range != 0 && cv->full_range != 1 ? OH_E_ARG : OH_OK;
}

/* the luma and chroma excursions of B-bit samples in full or limited range, and the luma offset */
static void range_scales(int full_range, int B, double *ys, double *cs, int *yoff)
{
    const double full = (double)((1 << B) - 1), unit = (double)(1 << (B - 8));
    *ys = full_range ? full : 219.0 * unit; *cs = full_range ? full : 224.0 * unit;
    *yoff = full_range ? 0 : 16 << (B - 8);
}

/* the integers of an RGB conversion: R = clamp((cy (Y - yoff) + crv (Cr - mid) + 2^(S-1)) >> S, 0, 2^D - 1), G with cgu, cgv, B with
 * cbu; each coefficient round(2^S (2^D - 1) entry / scale) of the H.273 inverse matrix, S the largest shift that keeps every term and
 * every sum inside int32 for all samples of bit_depth bits */
extern "C" int oh_convert_coeffs(const OhConvert *cv, int bit_depth, int32_t *out, int n)
{
    double kr, kb, ys, cs;
    { const int rc = coeffs_check(cv, bit_depth, out, n, OH_CONV_NCOEFFS, &kr, &kb); if (rc) return rc; }
    const int B = bit_depth, D = cv->sample == OH_CONV_U8 ? 8 : 16, mid = 1 << (B - 1);
    int yoff;
    range_scales(cv->full_range, B, &ys, &cs, &yoff);
    const double kg = 1.0 - kr - kb;
    const double ent[5] = { 1.0 / ys, 2.0 * (1.0 - kr) / cs, -2.0 * kb * (1.0 - kb) / (kg * cs), -2.0 * kr * (1.0 - kr) / (kg * cs),
                            2.0 * (1.0 - kb) / cs };              /* cy, crv, cgu, cgv, cbu */
    const int64_t dy = std::max(yoff, (1 << B) - 1 - yoff), dc = mid;   /* largest |Y - yoff|, |C - mid| */
    const double scale = (double)((1 << D) - 1);
    for (int S = 30; S >= 1; S--) {
        int64_t c[5];
        for (int i = 0; i < 5; i++) c[i] = llround(ldexp(scale * ent[i], S));
        const int64_t r = (int64_t)1 << (S - 1), ty = std::llabs(c[0]) * dy;
        const int64_t worst = std::max({ ty + std::llabs(c[1]) * dc + r, ty + (std::llabs(c[2]) + std::llabs(c[3])) * dc + r,
                                         ty + std::llabs(c[4]) * dc + r });
        if (worst > INT32_MAX)
            continue;
        for (int i = 0; i < 5; i++) out[i] = (int32_t)c[i];
        out[5] = yoff; out[6] = mid; out[7] = S; out[8] = D;
        return OH_OK;
    }
    return OH_E_UNSUPPORTED;
}

/* ---------------- import of standard images (import.hip) ---------------- */
/* the integers of an RGB import: Y = clamp((ry R + gy G + by B + (yoff << S) + 2^(S-1)) >> S, 0, 2^B - 1), Cb with the u row and mid,
 * Cr with the v row; each row sums to the exact scale (greys give mid, white gives peak luma); S the largest shift that keeps
 * (|c0| + |c1| + |c2|) (2^D - 1) + (offset << S) + 2^(S-1) of every row inside int32: every term and every partial sum, in whatever
 * order they are added */
extern "C" int oh_import_coeffs(const OhConvert *cv, int bit_depth, int32_t *out, int n)
{
    double kr, kb, ys, cs;
    { const int rc = coeffs_check(cv, bit_depth, out, n, OH_IMPORT_NCOEFFS, &kr, &kb); if (rc) return rc; }
    const int B = bit_depth, D = cv->sample == OH_CONV_U8 ? 8 : 16;
    int yoff32;
    range_scales(cv->full_range, B, &ys, &cs, &yoff32);
    const double M = (double)((1 << D) - 1);
    const int64_t yoff = yoff32, mid = 1 << (B - 1), Mi = ((int64_t)1 << D) - 1;
    for (int S = 30; S >= 1; S--) {
        int64_t c[9];
        c[0] = llround(ldexp(ys * kr / M, S));
        c[2] = llround(ldexp(ys * kb / M, S));
        c[1] = llround(ldexp(ys / M, S)) - c[0] - c[2];
        c[5] = c[6] = llround(ldexp(cs / (2.0 * M), S));
        c[3] = llround(ldexp(-cs * kr / (2.0 * (1.0 - kb) * M), S));
        c[4] = -c[3] - c[5];
        c[8] = llround(ldexp(-cs * kb / (2.0 * (1.0 - kr) * M), S));
        c[7] = -c[6] - c[8];
        const int64_t r = (int64_t)1 << (S - 1);
        int64_t worst = 0;
        for (int row = 0; row < 3; row++)
            worst = std::max<int64_t>(worst, (std::llabs(c[3 * row]) + std::llabs(c[3 * row + 1]) + std::llabs(c[3 * row + 2])) * Mi +
                                                 ((row ? mid : yoff) << S) + r);
        if (worst > INT32_MAX)
            continue;
        for (int i = 0; i < 9; i++) out[i] = (int32_t)c[i];
        out[9] = (int32_t)yoff; out[10] = (int32_t)mid; out[11] = S; out[12] = D;
        return OH_OK;
    }
    return OH_E_UNSUPPORTED;
}

/* ---------------- colour conversion (colour.hip) ---------------- */
namespace {
const double PQ_M1 = 2610.0 / 16384.0, PQ_M2 = 2523.0 / 4096.0 * 128.0, PQ_C1 = 3424.0 / 4096.0, PQ_C2 = 2413.0 / 4096.0 * 32.0,
             PQ_C3 = 2392.0 / 4096.0 * 32.0;
/* ST 2084: signal -> luminance / 10000 and back */
double pq_eotf(double x)
{
    const double xp = pow(std::max(x, 0.0), 1.0 / PQ_M2);
    return pow(std::max(xp - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * xp), 1.0 / PQ_M1);
}
double pq_inv(double y)
{
    const double yp = pow(std::max(y, 0.0), PQ_M1);
    return pow((PQ_C1 + PQ_C2 * yp) / (1.0 + PQ_C3 * yp), PQ_M2);
}
/* BT.2100 HLG inverse OETF: signal -> scene linear, 1 at signal 1 */
double hlg_inv_oetf(double x)
{
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    return x <= 0.5 ? x * x / 3.0 : (exp((x - c) / a) + b) / 12.0;
}
double srgb_eotf(double x) { return x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4); }
double srgb_inv(double l) { return l <= 0.0031308 ? 12.92 * l : 1.055 * pow(l, 1.0 / 2.4) - 0.055; }

bool is_sdr_video(int t) { return t == 1 || t == 6 || t == 14 || t == 15; }

/* BT.2390 EETF, black 0: nits -> nits.  Identity below the knee (exactly), the Hermite spline in the PQ domain above it, the target
 * peak from the source peak on (the spline ends there with slope 0) */
struct Eetf {
    double src_pq, mx, ks;
    Eetf(double src_peak, double dst_peak) : src_pq(pq_inv(src_peak / 10000.0)), mx(pq_inv(dst_peak / 10000.0) / src_pq), ks(1.5 * mx - 0.5) {}
    double gain(double nits) const
    {
        if (!(nits > 0))
            return 1.0;
        const double e1 = std::min(pq_inv(nits / 10000.0) / src_pq, 1.0);
        if (e1 <= ks)
            return 1.0;
        const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
        const double e2 = (2 * t3 - 3 * t2 + 1) * ks + (t3 - 2 * t2 + t) * (1.0 - ks) + (-2 * t3 + 3 * t2) * mx;
        return 10000.0 * pq_eotf(e2 * src_pq) / nits;
    }
};

void inv3(const double P[9], double inv[9])
{
    const double det = P[0] * (P[4] * P[8] - P[5] * P[7]) - P[1] * (P[3] * P[8] - P[5] * P[6]) + P[2] * (P[3] * P[7] - P[4] * P[6]);
    inv[0] = (P[4] * P[8] - P[5] * P[7]) / det; inv[1] = (P[2] * P[7] - P[1] * P[8]) / det; inv[2] = (P[1] * P[5] - P[2] * P[4]) / det;
    inv[3] = (P[5] * P[6] - P[3] * P[8]) / det; inv[4] = (P[0] * P[8] - P[2] * P[6]) / det; inv[5] = (P[2] * P[3] - P[0] * P[5]) / det;
    inv[6] = (P[3] * P[7] - P[4] * P[6]) / det; inv[7] = (P[1] * P[6] - P[0] * P[7]) / det; inv[8] = (P[0] * P[4] - P[1] * P[3]) / det;
}

/* linear RGB -> XYZ of a set of primaries with the D65 white, row-major; false: a code outside the list */
bool rgb_to_xyz(int prim, double m[9])
{
    double xy[6];
    switch (prim) {
    case 1:  { const double v[6] = { 0.640, 0.330, 0.300, 0.600, 0.150, 0.060 }; memcpy(xy, v, sizeof(v)); break; }
    case 9:  { const double v[6] = { 0.708, 0.292, 0.170, 0.797, 0.131, 0.046 }; memcpy(xy, v, sizeof(v)); break; }
    case 12: { const double v[6] = { 0.680, 0.320, 0.265, 0.690, 0.150, 0.060 }; memcpy(xy, v, sizeof(v)); break; }
    default: return false;
    }
    const double xw = 0.3127, yw = 0.3290, W[3] = { xw / yw, 1.0, (1.0 - xw - yw) / yw };
    double P[9];
    for (int i = 0; i < 3; i++) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        P[i] = x / y; P[3 + i] = 1.0; P[6 + i] = (1.0 - x - y) / y;
    }
    double inv[9];
    inv3(P, inv);
    for (int i = 0; i < 3; i++) {
        const double S = inv[3 * i] * W[0] + inv[3 * i + 1] * W[1] + inv[3 * i + 2] * W[2];
        for (int r = 0; r < 3; r++) m[3 * r + i] = P[3 * r + i] * S;
    }
    return true;
}

/* a row of fractions that sum to 1 with q fraction bits, the largest entry corrected so that the integers sum to exactly 2^q */
void q_row(const double r[3], int q, int32_t out[3])
{
    int best = 0, sum = 0;
    for (int j = 0; j < 3; j++) {
        out[j] = (int32_t)llround(ldexp(r[j], q));
        sum += out[j];
        if (out[j] > out[best]) best = j;
    }
    out[best] += (1 << q) - sum;
}

/* the node of entry k of a piecewise-logarithmic table, in units of 2^-30 of the full scale */
double node_of(int k) { return k < 128 ? (double)k : ldexp((double)(64 + (k & 63)), (k >> 6) - 1); }

/* rounded values into a table; false: a value, or a step between neighbours from entry `from` on (the entries the kernel interpolates
 * between), that its interpolation does not hold: max_step or more, or — rising — downwards */
bool narrow(const std::vector<double> &v, int32_t *out, int64_t max_step, size_t from, bool rising)
{
    int64_t prev = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (!std::isfinite(v[i]) || fabs(v[i]) > 2e9)
            return false;
        const int64_t r = llround(v[i]);
        if (i > from && (std::llabs(r - prev) >= max_step || (rising && r < prev)))
            return false;
        out[i] = (int32_t)r;
        prev = r;
    }
    return true;
}
}

/* what is wrong with an OhColour, by itself: OH_E_ARG, OH_E_UNSUPPORTED or OH_OK */
int colour_check(const OhColour *col, std::string *why)
{
    char buf[256];
    if (col->out_transfer < OH_COL_LINEAR || col->out_transfer > OH_COL_GAMMA24 || col->tone < OH_TONE_NONE || col->tone > OH_TONE_BT2390 ||
        col->norm < OH_NORM_MAXRGB || col->norm > OH_NORM_LUMA) {
        snprintf(buf, sizeof(buf), "out_transfer %d, tone %d or norm %d outside its list", col->out_transfer, col->tone, col->norm);
        *why = buf; return OH_E_ARG;
    }
    const float pk[3] = { col->src_peak, col->dst_peak, col->white };
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(pk[i]) || !(pk[i] > 0)) { *why = "src_peak, dst_peak and white are finite and positive"; return OH_E_ARG; }
    const int t = col->in_transfer;
    if (t != 16 && t != 18 && t != 13 && !is_sdr_video(t)) {
        snprintf(buf, sizeof(buf), "transfer_characteristics %d (16 PQ, 18 HLG, 13 sRGB, 1 / 6 / 14 / 15 SDR video)", t); *why = buf; return OH_E_UNSUPPORTED;
    }
    double m[9];
    if (!rgb_to_xyz(col->in_primaries, m) || !rgb_to_xyz(col->out_primaries, m)) {
        snprintf(buf, sizeof(buf), "colour_primaries %d -> %d (1 BT.709, 9 BT.2020, 12 P3-D65)", col->in_primaries, col->out_primaries);
        *why = buf; return OH_E_UNSUPPORTED;
    }
    if (t == 18 && col->norm == OH_NORM_MAXRGB) { *why = "HLG takes OH_NORM_LUMA: its OOTF is defined on luminance"; return OH_E_UNSUPPORTED; }
    if (t == 18 && !(col->src_peak >= 400.0f && col->src_peak <= 10000.0f)) { *why = "HLG with a nominal peak outside [400, 10000] nits"; return OH_E_UNSUPPORTED; }
    if (col->tone == OH_TONE_BT2390) {
        if (col->dst_peak >= col->src_peak) { *why = "OH_TONE_BT2390 with dst_peak >= src_peak"; return OH_E_UNSUPPORTED; }
        if (Eetf(col->src_peak, col->dst_peak).ks <= 0) { *why = "OH_TONE_BT2390 with a knee at or below black"; return OH_E_UNSUPPORTED; }
    }
    return OH_OK;
}

/* the tables in the layout of the device copy (tab: OH_COLT_N int32, zero-padded) and misc */
int colour_build(const OhColour *col, int32_t *tab, int32_t *misc, std::string *why)
{
    { const int rc = colour_check(col, why); if (rc) return rc; }
    const int t = col->in_transfer;
    const bool pq = t == 16, hlg = t == 18;
    const double Lfs = pq ? 10000.0 : (double)col->src_peak, src = col->src_peak, dstp = col->dst_peak;
    memset(tab, 0, (size_t)OH_COLT_N * sizeof(int32_t));
    memset(misc, 0, (size_t)OH_COL_NMISC * sizeof(int32_t));
    std::vector<double> v((size_t)OH_COL_NA);
    for (int i = 0; i < OH_COL_NA; i++) {
        const double x = 16.0 * i / 65535.0;
        v[i] = ldexp(pq ? pq_eotf(x) : hlg ? hlg_inv_oetf(x) : t == 13 ? srgb_eotf(x) : pow(x, 2.4), 30);
    }
    if (!narrow(v, tab, (int64_t)1 << 24, 0, true)) { *why = "the source curve's table falls or steps by 2^24 or more"; return OH_E_UNSUPPORTED; }
    const bool tone = col->tone == OH_TONE_BT2390;
    const double gamma = hlg ? 1.2 + 0.42 * log10(src / 1000.0) : 1.0;
    const Eetf tm(src, dstp);
    v.resize((size_t)OH_COL_NP);
    for (int k = 0; k < OH_COL_NP; k++) {
        const double x = ldexp(node_of(k), -30);
        double g = 1.0;
        if (hlg) g = x > 0 ? pow(x, gamma - 1.0) : 0.0;
        if (tone) g *= tm.gain(hlg ? src * pow(x, gamma) : Lfs * x);
        v[k] = ldexp(std::min(g, 1.0), 20);
    }
    if (!narrow(v, tab + OH_COLT_G, (int64_t)1 << 19, 128, false)) { *why = "the gain table steps by 2^19 or more"; return OH_E_UNSUPPORTED; }
    if (col->out_transfer != OH_COL_LINEAR) {
        for (int k = 0; k < OH_COL_NP; k++) {
            const double x = ldexp(node_of(k), -30) * Lfs / dstp;
            v[k] = 65535.0 * (col->out_transfer == OH_COL_SRGB ? srgb_inv(x) : pow(x, 1.0 / 2.4));
        }
        if (!narrow(v, tab + OH_COLT_B, (int64_t)1 << 19, 128, false)) { *why = "the output curve's table steps by 2^19 or more"; return OH_E_UNSUPPORTED; }
    }
    double si[9], so[9], soi[9];
    rgb_to_xyz(col->in_primaries, si);
    rgb_to_xyz(col->out_primaries, so);
    inv3(so, soi);
    for (int r = 0; r < 3; r++) {
        double row[3];
        for (int j = 0; j < 3; j++) row[j] = soi[3 * r] * si[j] + soi[3 * r + 1] * si[3 + j] + soi[3 * r + 2] * si[6 + j];
        q_row(row, 20, misc + 3 * r);
        if (col->in_primaries == col->out_primaries)
            for (int j = 0; j < 3; j++) misc[3 * r + j] = r == j ? 1 << 20 : 0;
    }
    q_row(si + 3, 14, misc + 9);
    misc[12] = col->norm;
    misc[13] = col->out_transfer != OH_COL_LINEAR;
    const float K = (float)(Lfs / ((double)col->white * 1073741824.0));
    if (!std::isfinite(K) || !(K > 0)) { *why = "white is out of the f32 range of the output scale"; return OH_E_UNSUPPORTED; }
    memcpy(&misc[14], &K, 4);
    misc[15] = hlg || tone;
    misc[16] = col->in_primaries != col->out_primaries;
    return OH_OK;
}

extern "C" int oh_colour_tables(const OhColour *col, int32_t *A, int32_t *G, int32_t *B, int32_t *misc)
{
    if (!col || !A || !G || !B || !misc)
        return OH_E_ARG;
    std::vector<int32_t> tab((size_t)OH_COLT_N);
    int32_t m[OH_COL_NMISC];
    std::string why;
    const int rc = colour_build(col, tab.data(), m, &why);
    if (rc) return rc;
    memcpy(A, tab.data(), (size_t)OH_COL_NA * 4);
    memcpy(G, tab.data() + OH_COLT_G, (size_t)OH_COL_NP * 4);
    memcpy(B, tab.data() + OH_COLT_B, (size_t)OH_COL_NP * 4);
    memcpy(misc, m, sizeof(m));
    return OH_OK;
}

/* ---------------- light-level statistics (light.hip) ---------------- */
extern "C" int oh_light_bin(uint32_t v)
{
    v = std::min(v, (uint32_t)1 << 30);
    if (v < (1u << 14))
        return 0;
    const int e = 31 - __builtin_clz(v);
    return 1 + 16 * (e - 14) + (int)((v >> (e - 4)) & 15);
}

extern "C" uint32_t oh_light_bin_upper(int bin)
{
    if (bin <= 0)
        return bin < 0 ? 0 : (1u << 14) - 1;
    if (bin >= OH_LL_NBINS)
        return 1u << 30;
    const int e = 14 + (bin - 1) / 16, j = (bin - 1) % 16;
    return (uint32_t)std::min<uint64_t>(((uint64_t)(17 + j) << (e - 4)) - 1, (uint64_t)1 << 30);
}

extern "C" int oh_light_percentile(const OhLightLevel *ll, int n, uint32_t ppm, uint32_t *value)
{
    if (!ll || !value || n < 1 || ppm > 1000000u)
        return OH_E_ARG;
    uint64_t total = 0;
    uint32_t top = 0;
    for (int i = 0; i < n; i++) {
        total += ll[i].pixels;
        top = std::max(top, ll[i].max);
    }
    if (!total)
        return OH_E_ARG;
    const uint64_t need = (uint64_t)ppm * total;
    uint64_t cum = 0;
    int b = 0;
    for (; b < OH_LL_NBINS - 1; b++) {                          /* histograms that hold fewer than `pixels` end in the last bin */
        for (int i = 0; i < n; i++) cum += ll[i].hist[b];
        if (cum * 1000000u >= need)
            break;
    }
    *value = std::min(oh_light_bin_upper(b), top);
    return OH_OK;
}

/* ---------------- comparison of two pictures (compare.hip) ---------------- */
extern "C" int oh_compare_ssim_consts(int bit_depth, int64_t *c1, int64_t *c2)
{
    if (!c1 || !c2 || !depth_ok(bit_depth))
        return OH_E_ARG;
    compare_ssim_consts(bit_depth, c1, c2);
    return OH_OK;
}

extern "C" int64_t oh_compare_ssim_window(int bit_depth, uint32_t s1, uint32_t s2, uint64_t ss, uint64_t s12)
{
    if (!depth_ok(bit_depth))
        return 0;
    int64_t c1, c2;
    compare_ssim_consts(bit_depth, &c1, &c2);
    return compare_ssim_window(c1, c2, s1, s2, ss, s12);
}

extern "C" double oh_compare_psnr(uint64_t sse, uint64_t samples, int bit_depth)
{
    if (!samples)
        return std::numeric_limits<double>::quiet_NaN();
    if (!sse)
        return std::numeric_limits<double>::infinity();
    const double M = (double)((1u << bit_depth) - 1);
    return 10.0 * std::log10(M * M * (double)samples / (double)sse);
}

/* ---------------- resizing into engine pictures (resize.hip) ---------------- */
typedef __int128 i128;
static i128 floor_div(i128 a, i128 b) { const i128 q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }   /* b > 0 */

static bool resize_axis_ok(int S, int T, int filter, int phase)
{
    return S >= 1 && T >= 1 && S <= 16384 && T <= 16384 && (filter == OH_RESIZE_BILINEAR || filter == OH_RESIZE_BICUBIC) && (phase == 1 || phase == 2);
}

extern "C" int oh_resize_max_taps(int src_extent, int dst_extent, int filter)
{
    if (!resize_axis_ok(src_extent, dst_extent, filter, 2))
        return OH_E_ARG;
    const int64_t S = src_extent, T = dst_extent, D = 4 * std::max(S, T), R = filter == OH_RESIZE_BICUBIC ? 2 : 1;
    return (int)std::min<int64_t>(S, (2 * R * D - 2) / (4 * T) + 1);          /* source samples strictly inside a span of 2RD */
}

/* the taps of one axis, all positions in units of 1/(4T) source samples */
extern "C" int oh_resize_taps(int src_extent, int dst_extent, int filter, int phase, int32_t *first, int16_t *coeffs, int max_taps, int *n_taps)
{
    if (!first || !coeffs || !n_taps || !resize_axis_ok(src_extent, dst_extent, filter, phase) ||
        max_taps < oh_resize_max_taps(src_extent, dst_extent, filter))
        return OH_E_ARG;
    const int64_t S = src_extent, T = dst_extent, p = phase, D = 4 * std::max(S, T), R = filter == OH_RESIZE_BICUBIC ? 2 : 1;
    std::vector<i128> w;
    std::vector<int64_t> k;
    for (int64_t x = 0; x < T; x++) {
        const int64_t c = (4 * x + p) * S;
        int64_t lo = -(int64_t)floor_div(-(c - R * D - p * T + 1), 4 * T), hi = (int64_t)floor_div(c + R * D - p * T - 1, 4 * T);
        lo = std::max<int64_t>(lo, 0); hi = std::min(hi, S - 1);
        const int n = (int)(hi - lo + 1);
        if (n < 1 || n > max_taps)
            return OH_E_ARG;
        w.assign((size_t)n, 0); k.assign((size_t)n, 0);
        i128 sum = 0;
        for (int j = 0; j < n; j++) {
            const i128 v = std::llabs((4 * (lo + j) + p) * T - c), d = D;
            w[j] = R == 1 ? d - v : v <= d ? 3 * v * v * v - 5 * v * v * d + 2 * d * d * d : -(v * v * v - 5 * v * v * d + 8 * v * d * d - 4 * d * d * d);
            sum += w[j];
        }
        if (sum <= 0)
            return OH_E_UNSUPPORTED;
        int64_t ks = 0, ka = 0;
        int best = 0;
        for (int j = 0; j < n; j++) {
            k[j] = (int64_t)floor_div(2 * w[j] * (1 << 14) + sum, 2 * sum);
            ks += k[j];
            if (k[j] > k[best]) best = j;
        }
        k[best] += (1 << 14) - ks;
        for (int j = 0; j < n; j++) ka += std::llabs(k[j]);
        if (ka >= 1 << 15)
            return OH_E_UNSUPPORTED;
        first[x] = (int32_t)lo; n_taps[x] = n;
        int16_t *row = coeffs + (size_t)x * max_taps;
        for (int j = 0; j < max_taps; j++) row[j] = j < n ? (int16_t)k[j] : 0;
    }
    return OH_OK;
}

/* ---------------- composition (compose.hip) ---------------- */
extern "C" uint32_t oh_compose_blend(uint32_t dst, uint32_t src, uint32_t alpha, uint32_t opacity)
{
    return compose_blend(dst, src, alpha, opacity);
}

extern "C" uint32_t oh_compose_chroma_alpha(int chroma_format_idc, uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11)
{
    return compose_chroma_alpha(chroma_format_idc, a00, a01, a10, a11);
}

/* ---------------- reformatting (reformat.hip) ---------------- */
extern "C" int32_t oh_reformat_quantise(int32_t sum, int s, int depth_mode, int x, int y, int dst_bit_depth)
{
    return reformat_quantise(sum, s, depth_mode, x, y, dst_bit_depth);
}

/* ---------------- orientation (orient.hip) ---------------- */
/* the definition on a small array whose samples all differ: transpose, then the horizontal flip, then the vertical one */
namespace {
struct Grid { int w, h, v[6]; };
const Grid GRID0 = { 3, 2, { 0, 1, 2, 3, 4, 5 } };
Grid grid_orient(const Grid &s, int o)
{
    Grid d = s;
    if (o & OH_ORIENT_TRANSPOSE) { d.w = s.h; d.h = s.w; }
    for (int y = 0; y < d.h; y++)
        for (int x = 0; x < d.w; x++) {
            const int ty = (o & OH_ORIENT_VFLIP) ? d.h - 1 - y : y, tx = (o & OH_ORIENT_HFLIP) ? d.w - 1 - x : x;
            d.v[y * d.w + x] = (o & OH_ORIENT_TRANSPOSE) ? s.v[tx * s.w + ty] : s.v[ty * s.w + tx];
        }
    return d;
}
}

extern "C" int oh_orient_then(int first, int second)
{
    if (first < 0 || first > 7 || second < 0 || second > 7)
        return -1;
    const Grid want = grid_orient(grid_orient(GRID0, first), second);
    for (int o = 0; o < 8; o++) {
        const Grid g = grid_orient(GRID0, o);
        if (g.w == want.w && g.h == want.h && !memcmp(g.v, want.v, sizeof(g.v)))
            return o;
    }
    return -1;
}

extern "C" int oh_orient_inverse(int orientation)
{
    for (int o = 0; o < 8; o++)
        if (oh_orient_then(orientation, o) == 0)
            return o;
    return -1;
}

extern "C" int oh_orient_size(int orientation, int w, int h, int *ow, int *oh)
{
    if (orientation < 0 || orientation > 7 || w < 1 || h < 1 || !ow || !oh)
        return OH_E_ARG;
    const bool t = orientation & OH_ORIENT_TRANSPOSE;
    *ow = t ? h : w; *oh = t ? w : h;
    return OH_OK;
}

extern "C" int oh_orient_from_sei(int hor_flip, int ver_flip, uint32_t anticlockwise_rotation, int *orientation)
{
    if (!orientation || hor_flip < 0 || hor_flip > 1 || ver_flip < 0 || ver_flip > 1 || anticlockwise_rotation > 0xFFFFu)
        return OH_E_ARG;
    if (anticlockwise_rotation & 0x3FFF)
        return OH_E_UNSUPPORTED;
    int o = (hor_flip ? OH_ORIENT_HFLIP : 0) | (ver_flip ? OH_ORIENT_VFLIP : 0);
    for (uint32_t k = anticlockwise_rotation >> 14; k; k--)
        o = oh_orient_then(o, OH_ORIENT_TRANSPOSE | OH_ORIENT_VFLIP);
    *orientation = o;
    return OH_OK;
}

/* ---------------- fields and deinterlacing (deinterlace.hip) ---------------- */
extern "C" int oh_field_info(int pic_struct, OhFieldInfo *out)
{
    if (!out || pic_struct < 0 || pic_struct > 12)
        return OH_E_ARG;
    /* H.265 Table D.2: 0 frame, 1 top, 2 bottom, 3 top-bottom, 4 bottom-top, 5 top-bottom-top, 6 bottom-top-bottom, 7 doubling,
     * 8 tripling, 9 top with previous bottom, 10 bottom with previous top, 11 top with next bottom, 12 bottom with next top */
    const int s = pic_struct;
    out->kind = s == 1 || s == 9 || s == 11 ? 1 : s == 2 || s == 10 || s == 12 ? 2 : 0;
    out->pair = s == 9 || s == 10 ? -1 : s == 11 || s == 12 ? 1 : 0;
    out->top_first = s == 3 || s == 5 ? 1 : s == 4 || s == 6 ? 0 : -1;
    out->repeat_first = s == 5 || s == 6;
    out->frames = s == 7 ? 2 : s == 8 ? 3 : 1;
    return OH_OK;
}

extern "C" int32_t oh_deint_adaptive(const int32_t up[7], const int32_t dn[7], int32_t a, int32_t b, int32_t pu, int32_t pd, int32_t nu, int32_t nd)
{
    return deint_adaptive(up, dn, a, b, pu, pd, nu, nd);
}

/* ---------------- filters (filter.hip) ---------------- */
extern "C" int oh_filter_taps_check(const OhFilterTaps *t)
{
    if (!t || t->nh < 1 || t->nh > OH_FILTER_MAX_TAPS || !(t->nh & 1) || t->nv < 1 || t->nv > OH_FILTER_MAX_TAPS || !(t->nv & 1))
        return OH_E_ARG;
    for (int axis = 0; axis < 2; axis++) {
        const int16_t *k = axis ? t->v : t->h;
        int sum = 0, mag = 0;
        for (int i = 0; i < (axis ? t->nv : t->nh); i++) { sum += k[i]; mag += std::abs((int)k[i]); }
        if (sum != 256 || mag > 512)
            return OH_E_ARG;
    }
    return OH_OK;
}

extern "C" int oh_filter_binomial(int n, int16_t *out)
{
    if (!out || n < 1 || n > 9 || !(n & 1))
        return OH_E_ARG;
    int row[9] = { 1 };
    for (int i = 1; i < n; i++)                                 /* row n - 1 of Pascal's triangle: its sum 2^(n - 1) divides 256 */
        for (int j = i; j > 0; j--) row[j] += row[j - 1];
    for (int j = 0; j < n; j++) out[j] = (int16_t)(row[j] * (256 >> (n - 1)));
    return OH_OK;
}

extern "C" int oh_filter_box(int n, int16_t *out)
{
    if (!out || n < 1 || n > OH_FILTER_MAX_TAPS || !(n & 1))
        return OH_E_ARG;
    for (int j = 0; j < n; j++) out[j] = (int16_t)(256 / n);
    out[n / 2] += (int16_t)(256 % n);
    return OH_OK;
}

extern "C" int32_t oh_filter_unsharp(int32_t s, int32_t b, int32_t amount, int32_t threshold, int32_t M)
{
    return filter_unsharp(s, b, amount, threshold, M);
}

extern "C" int32_t oh_filter_median9(const int32_t v[9]) { return filter_median9(v); }

extern "C" int32_t oh_filter_temporal(int32_t c, int32_t p, int32_t n, int32_t mp, int32_t mn, int32_t threshold)
{
    return filter_temporal(c, p, n, mp, mn, threshold);
}

/* what oh_pics_filter checks of the OhFilter itself, for pictures of bit_depth bits: the fields its mode reads, for both classes */
int filter_check(const OhFilter *f, int bit_depth, std::string *why)
{
    char buf[256];
    const int M = (1 << bit_depth) - 1;
    if (f->mode < OH_FILTER_CONVOLVE || f->mode > OH_FILTER_TEMPORAL) {
        snprintf(buf, sizeof(buf), "mode %d (0 convolve, 1 unsharp, 2 median, 3 temporal)", f->mode); *why = buf; return OH_E_ARG;
    }
    if (f->planes < 0 || f->planes > 7) { snprintf(buf, sizeof(buf), "planes %d (0 .. 7)", f->planes); *why = buf; return OH_E_ARG; }
    for (int q = 0; q < 2; q++) {
        if (f->mode <= OH_FILTER_UNSHARP && oh_filter_taps_check(&f->taps[q])) {
            snprintf(buf, sizeof(buf), "taps[%d]: %d x %d taps; each axis an odd number of 1 .. %d that sum to 256, their magnitudes to 512 at most",
                     q, f->taps[q].nh, f->taps[q].nv, (int)OH_FILTER_MAX_TAPS);
            *why = buf; return OH_E_ARG;
        }
        if (f->mode == OH_FILTER_UNSHARP && (f->amount[q] < -64 || f->amount[q] > 512)) {
            snprintf(buf, sizeof(buf), "amount[%d] %d (-64 .. 512)", q, f->amount[q]); *why = buf; return OH_E_ARG;
        }
        const int64_t top = f->mode == OH_FILTER_TEMPORAL ? 9 * (int64_t)M : M;
        if ((f->mode == OH_FILTER_UNSHARP || f->mode == OH_FILTER_TEMPORAL) && (f->threshold[q] < 0 || f->threshold[q] > top)) {
            snprintf(buf, sizeof(buf), "threshold[%d] %d (0 .. %lld)", q, f->threshold[q], (long long)top); *why = buf; return OH_E_ARG;
        }
    }
    return OH_OK;
}

/* ---------------- histograms and look-up tables (histogram.hip, lut.hip) ---------------- */
/* the fields of a plane's histogram that follow from its bins (the kernel makes nothing else), in 64-bit integers */
void hist_derive(const uint32_t *bins, OhPlaneHist *out)
{
    memset(out, 0, sizeof(*out));
    bool any = false;
    for (uint32_t v = 0; v < OH_HIST_BINS; v++) {
        const uint64_t c = bins[v];
        out->hist[v] = bins[v];
        if (!c)
            continue;
        out->samples += c;
        out->sum += c * v;
        out->sum_sq += c * v * v;
        if (!any) out->min = v;
        out->max = v;
        any = true;
    }
}

/* the pooled count of bin v of n histograms */
static uint64_t pooled(const OhPlaneHist *h, int n, int v)
{
    uint64_t c = 0;
    for (int i = 0; i < n; i++) c += h[i].hist[v];
    return c;
}

static uint64_t pooled_total(const OhPlaneHist *h, int n)
{
    uint64_t N = 0;
    for (int v = 0; v < OH_HIST_BINS; v++) N += pooled(h, n, v);
    return N;
}

extern "C" int oh_hist_percentile(const OhPlaneHist *h, int n, uint32_t ppm, uint32_t *value)
{
    if (!h || !value || n < 1 || ppm > 1000000u)
        return OH_E_ARG;
    const uint64_t N = pooled_total(h, n);
    if (!N)
        return OH_E_ARG;
    const uint64_t need = (uint64_t)ppm * N;
    uint64_t cum = 0;
    for (int v = 0; v < OH_HIST_BINS; v++) {
        cum += pooled(h, n, v);
        if (cum && cum * 1000000u >= need) {
            *value = (uint32_t)v;
            return OH_OK;
        }
    }
    return OH_E_ARG;                                            /* not reached: cum ends at N */
}

extern "C" int oh_hist_distance(const OhPlaneHist *a, const OhPlaneHist *b, uint64_t *sad)
{
    if (!a || !b || !sad)
        return OH_E_ARG;
    uint64_t s = 0;
    for (int v = 0; v < OH_HIST_BINS; v++)
        s += a->hist[v] > b->hist[v] ? a->hist[v] - b->hist[v] : b->hist[v] - a->hist[v];
    *sad = s;
    return OH_OK;
}

extern "C" int oh_lut_identity(int bs, int bd, uint16_t *out)
{
    if (!depth_ok(bs) || !depth_ok(bd) || !out)
        return OH_E_ARG;
    for (int v = 0; v < (1 << bs); v++)
        out[v] = (uint16_t)reformat_quantise(v, bs - bd, OH_RF_ROUND, 0, 0, bd);
    return OH_OK;
}

extern "C" int oh_lut_range(int bs, int bd, int to_full, int chroma, uint16_t *out)
{
    if (!depth_ok(bs) || !depth_ok(bd) || !out)
        return OH_E_ARG;
    const int64_t Ms = (1 << bs) - 1, Md = (1 << bd) - 1, ks = 1 << (bs - 8), kd = 1 << (bd - 8);
    for (int64_t v = 0; v <= Ms; v++) {
        int64_t o;
        if (to_full && !chroma) {
            const int64_t c = std::min(std::max(v, 16 * ks), 235 * ks) - 16 * ks;
            o = (c * Md + (219 * ks >> 1)) / (219 * ks);
        } else if (to_full) {
            const int64_t d = std::min(std::max(v, 16 * ks), 240 * ks) - 128 * ks;
            const int64_t m = ((d < 0 ? -d : d) * Md + 112 * ks) / (224 * ks);
            o = std::min(std::max(((int64_t)1 << (bd - 1)) + (d < 0 ? -m : m), (int64_t)0), Md);
        } else if (!chroma) {
            o = 16 * kd + (v * 219 * kd + (Ms >> 1)) / Ms;
        } else {
            const int64_t d = v - ((int64_t)1 << (bs - 1));
            const int64_t m = ((d < 0 ? -d : d) * 224 * kd + (Ms >> 1)) / Ms;
            o = std::min(std::max(128 * kd + (d < 0 ? -m : m), 16 * kd), 240 * kd);
        }
        out[v] = (uint16_t)o;
    }
    return OH_OK;
}

extern "C" int oh_lut_linear(int bs, int bd, int32_t gain_q16, int32_t pivot_in, int32_t pivot_out, uint16_t *out)
{
    if (!depth_ok(bs) || !depth_ok(bd) || !out)
        return OH_E_ARG;
    const int64_t Md = (1 << bd) - 1;
    for (int64_t v = 0; v < (1 << bs); v++) {                   /* |v - pivot_in| <= 2^31 + 4095 and |gain| <= 2^31: the sum stays below 2^63 */
        const int64_t y = ((v - pivot_in) * gain_q16 + (int64_t)pivot_out * 65536 + 32768) >> 16;
        out[v] = (uint16_t)std::min(std::max(y, (int64_t)0), Md);
    }
    return OH_OK;
}

extern "C" int oh_lut_stretch(const OhPlaneHist *h, int n, uint32_t lo_ppm, uint32_t hi_ppm, int bd, uint16_t *out)
{
    if (!h || n < 1 || !depth_ok(bd) || !out || (uint64_t)lo_ppm + hi_ppm >= 1000000u)
        return OH_E_ARG;
    uint32_t lo32 = 0, hi32 = 0;
    if (oh_hist_percentile(h, n, lo_ppm, &lo32) || oh_hist_percentile(h, n, 1000000u - hi_ppm, &hi32))
        return OH_E_ARG;
    const int64_t lo = lo32, hi = hi32, M = (1 << bd) - 1;
    for (int64_t v = 0; v <= M; v++)
        out[v] = (uint16_t)(hi <= lo ? v : ((std::min(std::max(v, lo), hi) - lo) * M + ((hi - lo) >> 1)) / (hi - lo));
    return OH_OK;
}

extern "C" int oh_lut_equalise(const OhPlaneHist *h, int n, int bd, uint16_t *out)
{
    if (!h || n < 1 || !depth_ok(bd) || !out)
        return OH_E_ARG;
    const uint64_t N = pooled_total(h, n), M = (1u << bd) - 1;
    uint64_t cmin = 0;
    for (int v = 0; v < OH_HIST_BINS && !cmin; v++) cmin = pooled(h, n, v);
    uint64_t cum = 0;
    for (uint64_t v = 0; v <= M; v++) {
        cum += pooled(h, n, (int)v);
        out[v] = (uint16_t)(N == cmin ? v : cum < cmin ? 0 : ((cum - cmin) * M + ((N - cmin) >> 1)) / (N - cmin));
    }
    return OH_OK;
}

extern "C" int oh_lut_then(const uint16_t *first, int n1, const uint16_t *second, int n2, uint16_t *out)
{
    if (!first || !second || !out || n1 < 1 || n2 < 1)
        return OH_E_ARG;
    for (int v = 0; v < n1; v++)
        if (first[v] >= n2)
            return OH_E_ARG;
    for (int v = 0; v < n1; v++)
        out[v] = second[first[v]];
    return OH_OK;
}

/* what oh_pics_lut checks of the OhLut itself (planes is in 0 .. 7), for sources of sbd and destinations of dbd bits with np planes */
int lut_check(const OhLut *lut, int sbd, int dbd, int np, std::string *why)
{
    char buf[256];
    if (lut->n_entries != 1 << sbd) {
        snprintf(buf, sizeof(buf), "n_entries %d for sources of %d bits (%d)", lut->n_entries, sbd, 1 << sbd); *why = buf; return OH_E_ARG;
    }
    for (int c = 0; c < np; c++) {
        if (!(lut->planes >> c & 1)) {
            if (sbd != dbd) {
                snprintf(buf, sizeof(buf), "plane %d is copied, from %d to %d bits", c, sbd, dbd); *why = buf; return OH_E_ARG;
            }
            continue;
        }
        if (!lut->table[c]) { snprintf(buf, sizeof(buf), "no table for plane %d", c); *why = buf; return OH_E_ARG; }
        for (int v = 0; v < lut->n_entries; v++)
            if (lut->table[c][v] >> dbd) {
                snprintf(buf, sizeof(buf), "table[%d][%d] = %d does not fit %d bits", c, v, lut->table[c][v], dbd); *why = buf; return OH_E_ARG;
            }
    }
    return OH_OK;
}

/* ---------------- motion: the host-only helpers and what oh_pics_motion checks ---------------- */
static bool block_ok(int block) { return block == 8 || block == 16; }

extern "C" int oh_motion_blocks(int width, int height, int block, int *bw, int *bh)
{
    if (width < 1 || height < 1 || !block_ok(block) || !bw || !bh)
        return OH_E_ARG;
    *bw = (width + block - 1) / block; *bh = (height + block - 1) / block;
    return OH_OK;
}

extern "C" int oh_motion_scale(const OhMotionVector *coarse, int bwc, int bhc, int block_c, int s, int bw, int bh, int block_f, int16_t *centres)
{
    if (!coarse || !centres || bwc < 1 || bhc < 1 || bw < 1 || bh < 1 || !block_ok(block_c) || !block_ok(block_f) ||
        (s != 1 && s != 2 && s != 4 && s != 8))
        return OH_E_ARG;
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            const int64_t span = (int64_t)s * block_c;
            const int64_t qx = std::min<int64_t>((int64_t)bx * block_f / span, bwc - 1), qy = std::min<int64_t>((int64_t)by * block_f / span, bhc - 1);
            const OhMotionVector &v = coarse[qy * bwc + qx];
            const int comp[2] = { v.x, v.y };
            for (int k = 0; k < 2; k++)
                centres[2 * ((size_t)by * bw + bx) + k] =
                    (int16_t)std::min(std::max((s * comp[k] + 2) >> 2, -(int)OH_MOTION_MAX_CENTRE), (int)OH_MOTION_MAX_CENTRE);
        }
    return OH_OK;
}

extern "C" int32_t oh_motion_qpel(const uint16_t win[64], int fx, int fy, int bit_depth)
{
    if (!win || fx < 0 || fx > 3 || fy < 0 || fy > 3 || !depth_ok(bit_depth))
        return -1;
    return motion_sample<8>(win, 8, fx, fy, bit_depth);
}

extern "C" int32_t oh_motion_epel(const uint16_t win[16], int fx, int fy, int bit_depth)
{
    if (!win || fx < 0 || fx > 7 || fy < 0 || fy > 7 || !depth_ok(bit_depth))
        return -1;
    return motion_sample<4>(win, 4, fx, fy, bit_depth);
}

extern "C" uint64_t oh_motion_cost(uint32_t sad, int mvx, int mvy, int cx, int cy, int lambda)
{
    const int64_t dx = (int64_t)mvx - 4 * (int64_t)cx, dy = (int64_t)mvy - 4 * (int64_t)cy;
    const int64_t d = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    return (uint64_t)((int64_t)sad + (((int64_t)lambda * d) >> 2));
}

/* what oh_pics_motion checks of the OhMotionSearch itself; n_centres: the (cx, cy) pairs the call reads of ms->centres, if it has any */
int motion_check(const OhMotionSearch *ms, size_t n_centres, std::string *why)
{
    char buf[256];
    if (!block_ok(ms->block)) { snprintf(buf, sizeof(buf), "block %d (8 or 16)", ms->block); *why = buf; return OH_E_ARG; }
    if (ms->range_x < 0 || ms->range_x > OH_MOTION_MAX_RANGE || ms->range_y < 0 || ms->range_y > OH_MOTION_MAX_RANGE) {
        snprintf(buf, sizeof(buf), "range %d x %d outside 0 .. %d", ms->range_x, ms->range_y, OH_MOTION_MAX_RANGE); *why = buf; return OH_E_ARG;
    }
    if (ms->subpel < 0 || ms->subpel > 2) { snprintf(buf, sizeof(buf), "subpel %d (0 integer, 1 half, 2 quarter)", ms->subpel); *why = buf; return OH_E_ARG; }
    if (ms->lambda < 0 || ms->lambda > OH_MOTION_MAX_LAMBDA) {
        snprintf(buf, sizeof(buf), "lambda %d outside 0 .. %d", ms->lambda, OH_MOTION_MAX_LAMBDA); *why = buf; return OH_E_ARG;
    }
    if (ms->centres)
        for (size_t i = 0; i < 2 * n_centres; i++)
            if (ms->centres[i] < -OH_MOTION_MAX_CENTRE || ms->centres[i] > OH_MOTION_MAX_CENTRE) {
                snprintf(buf, sizeof(buf), "centre %zu is (%d, %d): beyond %d", i / 2, ms->centres[i & ~(size_t)1], ms->centres[i | 1], OH_MOTION_MAX_CENTRE);
                *why = buf; return OH_E_ARG;
            }
    return OH_OK;
}

/* ---------------- warping: the host-only helpers and what oh_pics_warp checks ---------------- */
static bool within(int64_t v, int bits) { return v >= -((int64_t)1 << bits) && v <= ((int64_t)1 << bits); }

/* the mode and the coefficients it reads */
int warp_map_check(const OhWarp *w, std::string *why)
{
    char buf[256];
    if (w->mode < OH_WARP_AFFINE || w->mode > OH_WARP_PERSPECTIVE) {
        snprintf(buf, sizeof(buf), "mode %d (0 affine, 1 perspective)", w->mode); *why = buf; return OH_E_ARG;
    }
    const int64_t *m = w->m;
    if (!within(m[0], 22) || !within(m[1], 22) || !within(m[3], 22) || !within(m[4], 22) || !within(m[2], 36) || !within(m[5], 36)) {
        *why = "m[0], m[1], m[3], m[4] beyond 2^22 or m[2], m[5] beyond 2^36 (Q16)"; return OH_E_ARG;
    }
    if (w->mode == OH_WARP_PERSPECTIVE && (!within(m[6], 26) || !within(m[7], 26) || m[8] <= 0 || m[8] > (int64_t)1 << 36)) {
        *why = "m[6], m[7] beyond 2^26 or m[8] outside 1 .. 2^36 (Q30)"; return OH_E_ARG;
    }
    return OH_OK;
}

/* the perspective denominator at luma sample (X, Y), at least 2^20 */
static bool warp_denominator_ok(const OhWarp *w, int64_t X, int64_t Y)
{
    return w->mode != OH_WARP_PERSPECTIVE || w->m[6] * X + w->m[7] * Y + w->m[8] >= (int64_t)1 << 20;
}

/* what oh_pics_warp checks of the OhWarp itself, without pictures; the image is checked where width is not 0 */
int warp_check(const OhWarp *w, int bit_depth, std::string *why)
{
    char buf[256];
    { const int rc = warp_map_check(w, why); if (rc) return rc; }
    if (w->filter < OH_WARP_NEAREST || w->filter > OH_WARP_BICUBIC) {
        snprintf(buf, sizeof(buf), "filter %d (0 nearest, 1 bilinear, 2 bicubic)", w->filter); *why = buf; return OH_E_ARG;
    }
    if (w->border < OH_WARP_REPLICATE || w->border > OH_WARP_CONSTANT) {
        snprintf(buf, sizeof(buf), "border %d (0 replicate, 1 constant)", w->border); *why = buf; return OH_E_ARG;
    }
    if (w->border == OH_WARP_CONSTANT)
        for (int c = 0; c < 3; c++)
            if (w->fill[c] >> bit_depth) {
                snprintf(buf, sizeof(buf), "fill[%d] = %d does not fit %d bits", c, w->fill[c], bit_depth); *why = buf; return OH_E_ARG;
            }
    return OH_OK;
}

/* the image of a call: inside 1 .. 16384, and the denominator at its four corner samples */
int warp_image_check(const OhWarp *w, std::string *why)
{
    char buf[256];
    if (w->width < 1 || w->height < 1 || w->width > 16384 || w->height > 16384) {
        snprintf(buf, sizeof(buf), "image %dx%d: outside 1 .. 16384", w->width, w->height); *why = buf; return OH_E_ARG;
    }
    for (int k = 0; k < 4; k++)
        if (!warp_denominator_ok(w, k & 1 ? w->width - 1 : 0, k & 2 ? w->height - 1 : 0)) {
            snprintf(buf, sizeof(buf), "the perspective denominator is below 2^20 at corner (%d, %d) of the image", k & 1 ? w->width - 1 : 0,
                     k & 2 ? w->height - 1 : 0);
            *why = buf; return OH_E_ARG;
        }
    return OH_OK;
}

extern "C" int oh_warp_position(const OhWarp *w, int hs, int vs, int x, int y, int32_t *px_q16, int32_t *py_q16)
{
    std::string why;
    if (!w || !px_q16 || !py_q16 || hs < 0 || hs > 1 || vs < 0 || vs > 1 || x < 0 || y < 0 || x > 16384 >> hs || y > 16384 >> vs || warp_map_check(w, &why))
        return OH_E_ARG;
    if (w->mode == OH_WARP_PERSPECTIVE) {
        if (w->m[6] * ((int64_t)x << hs) + w->m[7] * ((int64_t)y << vs) + w->m[8] + vs * (w->m[7] >> 1) < (int64_t)1 << 20)
            return OH_E_ARG;
        warp_position<true>(w->m, hs, vs, x, y, px_q16, py_q16);
    } else
        warp_position<false>(w->m, hs, vs, x, y, px_q16, py_q16);
    return OH_OK;
}

extern "C" int oh_warp_cubic(int f, int16_t c[4])
{
    if (f < 0 || f > 63 || !c)
        return OH_E_ARG;
    int32_t k[4];
    warp_cubic(f, k);
    for (int i = 0; i < 4; i++) c[i] = (int16_t)k[i];
    return OH_OK;
}

extern "C" int32_t oh_warp_interp(const uint16_t taps[16], int fx, int fy, int filter, int bit_depth)
{
    if (!taps || fx < 0 || fx > 63 || fy < 0 || fy > 63 || filter < OH_WARP_NEAREST || filter > OH_WARP_BICUBIC || !depth_ok(bit_depth))
        return -1;
    return warp_interp(filter, [=](int i, int j) { return (int32_t)taps[4 * j + i]; }, 1, 1, fx, fy, (1 << bit_depth) - 1);
}

extern "C" int oh_warp_paths(const OhWarp *w, int bit_depth, int chroma_format_idc, int dst_width, int dst_height, int64_t *staged, int64_t *gathered)
{
    std::string why;
    const int cf = chroma_format_idc, hs = cf == 1 || cf == 2, vs = cf == 1;
    if (!w || !staged || !gathered || !depth_ok(bit_depth) || cf < 0 || cf > 3 || warp_check(w, bit_depth, &why) || warp_image_check(w, &why) ||
        w->width > dst_width || w->height > dst_height || dst_width > 16384 || dst_height > 16384 || w->width % (1 << hs) || w->height % (1 << vs) ||
        dst_width % (1 << hs) || dst_height % (1 << vs))
        return OH_E_ARG;
    *staged = *gathered = 0;
    for (int q = 0; q < (cf ? 2 : 1); q++) {
        const int sx = q ? hs : 0, sy = q ? vs : 0, dw = dst_width >> sx, dh = dst_height >> sy, iw = w->width >> sx, ih = w->height >> sy;
        for (int ty = 0; ty * WARP_TH < dh; ty++)
            for (int tx = 0; tx * WARP_TW < dw; tx++) {
                int xa, ya, xb, yb;
                warp_tile_corners(tx, ty, dw, dh, iw, ih, &xa, &ya, &xb, &yb);
                const WarpBox b = w->mode == OH_WARP_PERSPECTIVE ? warp_tile_box<true>(w->m, sx, sy, w->filter, xa, ya, xb, yb)
                                                                 : warp_tile_box<false>(w->m, sx, sy, w->filter, xa, ya, xb, yb);
                *(warp_box_staged(b, bit_depth > 8 ? 2 : 1) ? staged : gathered) += q ? 2 : 1;
            }
    }
    return OH_OK;
}

extern "C" int oh_warp_identity(OhWarp *out)
{
    if (!out)
        return OH_E_ARG;
    memset(out, 0, sizeof(*out));
    out->mode = OH_WARP_AFFINE; out->filter = OH_WARP_BILINEAR; out->border = OH_WARP_REPLICATE;
    out->m[0] = out->m[4] = 65536;
    out->m[8] = (int64_t)1 << 30;
    return OH_OK;
}

extern "C" int oh_warp_translation(int32_t dx_q2, int32_t dy_q2, OhWarp *out)
{
    if (oh_warp_identity(out))
        return OH_E_ARG;
    out->m[2] = (int64_t)dx_q2 * 16384;
    out->m[5] = (int64_t)dy_q2 * 16384;
    return OH_OK;
}

static bool warp_affine_ok(const OhWarp *w)
{
    std::string why;
    return w && w->mode == OH_WARP_AFFINE && !warp_map_check(w, &why);
}

extern "C" int oh_warp_then(const OhWarp *first, const OhWarp *second, OhWarp *out)
{
    if (!out || !warp_affine_ok(first) || !warp_affine_ok(second))
        return OH_E_ARG;
    const int64_t *a = first->m, *b = second->m;
    auto P = [](int64_t x, int64_t y) { return (x * y + 32768) >> 16; };
    OhWarp r = *first;
    r.width = second->width; r.height = second->height;
    r.m[0] = P(a[0], b[0]) + P(a[1], b[3]);
    r.m[1] = P(a[0], b[1]) + P(a[1], b[4]);
    r.m[2] = P(a[0], b[2]) + P(a[1], b[5]) + a[2];
    r.m[3] = P(a[3], b[0]) + P(a[4], b[3]);
    r.m[4] = P(a[3], b[1]) + P(a[4], b[4]);
    r.m[5] = P(a[3], b[2]) + P(a[4], b[5]) + a[5];
    r.m[6] = r.m[7] = 0; r.m[8] = (int64_t)1 << 30;
    if (!warp_affine_ok(&r))
        return OH_E_ARG;
    *out = r;
    return OH_OK;
}

/* n / d rounded to nearest, halves up; d != 0.  false: the quotient leaves 63 bits */
static bool rounded_div(__int128 n, __int128 d, int64_t *q)
{
    if (d < 0) { n = -n; d = -d; }
    const __int128 t = 2 * n + d, dd = 2 * d;
    __int128 r = t / dd;
    if (t % dd < 0) r--;
    if (r > ((__int128)1 << 62) || r < -((__int128)1 << 62))
        return false;
    *q = (int64_t)r;
    return true;
}

extern "C" int oh_warp_invert(const OhWarp *fwd, OhWarp *out)
{
    if (!out || !warp_affine_ok(fwd))
        return OH_E_ARG;
    const __int128 a = fwd->m[0], b = fwd->m[1], tx = fwd->m[2], c = fwd->m[3], d = fwd->m[4], ty = fwd->m[5];
    const __int128 det = a * d - b * c, one = (__int128)1 << 32, q16 = 65536;
    if (det == 0)
        return OH_E_ARG;
    OhWarp r = *fwd;
    if (!rounded_div(d * one, det, &r.m[0]) || !rounded_div(-b * one, det, &r.m[1]) || !rounded_div((b * ty - d * tx) * q16, det, &r.m[2]) ||
        !rounded_div(-c * one, det, &r.m[3]) || !rounded_div(a * one, det, &r.m[4]) || !rounded_div((c * tx - a * ty) * q16, det, &r.m[5]))
        return OH_E_ARG;
    r.m[6] = r.m[7] = 0; r.m[8] = (int64_t)1 << 30;
    if (!warp_affine_ok(&r))
        return OH_E_ARG;
    *out = r;
    return OH_OK;
}

extern "C" int oh_warp_rotation(uint32_t anticlockwise, int64_t cx_src_q16, int64_t cy_src_q16, int64_t cx_dst_q16, int64_t cy_dst_q16,
                                int32_t scale_q16, OhWarp *out)
{
    if (!out || anticlockwise >= 65536u || scale_q16 < 1 || scale_q16 > 1 << 22 || !within(cx_src_q16, 36) || !within(cy_src_q16, 36) ||
        !within(cx_dst_q16, 36) || !within(cy_dst_q16, 36))
        return OH_E_ARG;
    int64_t co, si;
    if (!(anticlockwise & 0x3FFF)) {
        const int k = (int)(anticlockwise >> 14);
        co = k == 0 ? scale_q16 : k == 2 ? -(int64_t)scale_q16 : 0;
        si = k == 1 ? scale_q16 : k == 3 ? -(int64_t)scale_q16 : 0;
    } else {
        const double t = (double)anticlockwise * (6.283185307179586476925286766559 / 65536.0);
        co = llrint((double)scale_q16 * cos(t));
        si = llrint((double)scale_q16 * sin(t));
    }
    OhWarp r;
    (void)oh_warp_identity(&r);
    r.m[0] = co; r.m[1] = -si; r.m[3] = si; r.m[4] = co;
    r.m[2] = cx_src_q16 - ((r.m[0] * cx_dst_q16 + r.m[1] * cy_dst_q16 + 32768) >> 16);
    r.m[5] = cy_src_q16 - ((r.m[3] * cx_dst_q16 + r.m[4] * cy_dst_q16 + 32768) >> 16);
    if (!warp_affine_ok(&r))
        return OH_E_ARG;
    *out = r;
    return OH_OK;
}

extern "C" int oh_warp_from_sei(int hor_flip, int ver_flip, uint32_t anticlockwise_rotation, int w, int h, OhWarp *out, int *ow, int *oh)
{
    if (!out || !ow || !oh || hor_flip < 0 || hor_flip > 1 || ver_flip < 0 || ver_flip > 1 || anticlockwise_rotation >= 65536u || w < 1 || h < 1 ||
        w > 16384 || h > 16384)
        return OH_E_ARG;
    OhWarp r;
    if (oh_warp_rotation(anticlockwise_rotation, 0, 0, 0, 0, 65536, &r))
        return OH_E_ARG;
    auto mag = [](int64_t v) { return v < 0 ? -v : v; };
    const int iw = (int)(((mag(r.m[0]) * w + mag(r.m[1]) * h + 65535) >> 16) + 1) & ~1, ih = (int)(((mag(r.m[3]) * w + mag(r.m[4]) * h + 65535) >> 16) + 1) & ~1;
    if (oh_warp_rotation(anticlockwise_rotation, (int64_t)(w - 1) << 15, (int64_t)(h - 1) << 15, (int64_t)(iw - 1) << 15, (int64_t)(ih - 1) << 15, 65536, &r))
        return OH_E_ARG;
    if (hor_flip) { r.m[0] = -r.m[0]; r.m[1] = -r.m[1]; r.m[2] = ((int64_t)(w - 1) << 16) - r.m[2]; }
    if (ver_flip) { r.m[3] = -r.m[3]; r.m[4] = -r.m[4]; r.m[5] = ((int64_t)(h - 1) << 16) - r.m[5]; }
    r.width = iw; r.height = ih;
    *out = r;
    *ow = iw; *oh = ih;
    return OH_OK;
}

/* ---------------- film grain (grain.hip): the host-only helpers and what oh_pics_grain checks ---------------- */
static bool cut_ok(int f) { return f >= GRAIN_CUT_MIN && f <= GRAIN_CUT_MAX; }

extern "C" uint32_t oh_grain_hash(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return grain_hash(a, b, c, d); }
extern "C" int32_t oh_grain_gauss(uint32_t h) { return grain_gauss(h); }

/* one stage of HEVC's inverse 32-point transform over all 32 lines of c: down the columns (pass 0) or along the rows (pass 1) */
static void grain_inverse_stage(int16_t *c, int pass, int shift)
{
    static const int8_t cosv[32] = { 64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67,
                                     64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4 };
    int m[32][32];                                              /* row k: the basis function of frequency k */
    for (int k = 0; k < 32; k++)
        for (int n = 0; n < 32; n++) {
            int a = (k * (2 * n + 1)) & 127;
            if (a > 64) a = 128 - a;
            m[k][n] = k == 0 ? 64 : a == 32 ? 0 : a < 32 ? cosv[a] : -cosv[64 - a];
        }
    const int step = pass ? 1 : 32, line_step = pass ? 32 : 1;
    for (int line = 0; line < 32; line++) {
        int16_t *p = c + line * line_step;
        int32_t out[32];
        for (int i = 0; i < 32; i++) {
            int32_t acc = 0;
            for (int k = 0; k < 32; k++)
                acc += m[k][i] * p[k * step];
            acc = (acc + (1 << (shift - 1))) >> shift;
            out[i] = std::min(std::max(acc, -32768), 32767);
        }
        for (int i = 0; i < 32; i++)
            p[i * step] = (int16_t)out[i];
    }
}

extern "C" int oh_grain_pattern(int fh, int fv, int16_t *coeffs, int16_t *raw, int8_t *pattern)
{
    if (!cut_ok(fh) || !cut_ok(fv))
        return OH_E_ARG;
    int16_t c[GRAIN_PAT * GRAIN_PAT];
    for (int v = 0; v < GRAIN_PAT; v++)
        for (int u = 0; u < GRAIN_PAT; u++)
            c[v * GRAIN_PAT + u] = (u < 2 * fh && v < 2 * fv && (u || v))
                                       ? (int16_t)(8 * grain_gauss(grain_hash(1, (uint32_t)(fh * 16 + fv), (uint32_t)u, (uint32_t)v))) : (int16_t)0;
    if (coeffs) memcpy(coeffs, c, sizeof(c));
    grain_inverse_stage(c, 0, 7);
    grain_inverse_stage(c, 1, 12);                              /* 20 - bit depth, at 8 bit */
    if (raw) memcpy(raw, c, sizeof(c));
    if (!pattern)
        return OH_OK;
    int64_t ss = 0;
    for (int i = 0; i < GRAIN_PAT * GRAIN_PAT; i++)
        ss += (int64_t)c[i] * c[i];
    ss /= GRAIN_PAT * GRAIN_PAT;
    int64_t r = 0;
    while ((r + 1) * (r + 1) <= ss) r++;                        /* at most 32767 steps */
    for (int i = 0; i < GRAIN_PAT * GRAIN_PAT; i++) {
        int64_t v = 0;
        if (r) {
            const int64_t num = 64 * (int64_t)c[i] + r, den = 2 * r;
            v = num / den - (num % den < 0);                    /* floor */
        }
        pattern[i] = (int8_t)std::min<int64_t>(std::max<int64_t>(v, -127), 127);
    }
    return OH_OK;
}

extern "C" int oh_grain_uniform(int sigma, int fh, int fv, uint32_t *out)
{
    if (!out || sigma < 0 || sigma > 255 || !cut_ok(fh) || !cut_ok(fv))
        return OH_E_ARG;
    for (int a = 0; a < OH_GRAIN_ENTRIES; a++)
        out[a] = (uint32_t)sigma | (uint32_t)fh << 8 | (uint32_t)fv << 12;
    return OH_OK;
}

extern "C" int oh_grain_from_sei(const OhFilmGrainSei *sei, uint32_t tables[3][256], OhGrain *out)
{
    if (!sei || !tables || !out || !sei->present || sei->cancel)
        return OH_E_ARG;
    if (sei->model_id != 0 || sei->blending_mode_id < 0 || sei->blending_mode_id > 1 || sei->log2_scale_factor < 0 || sei->log2_scale_factor > 15)
        return OH_E_UNSUPPORTED;
    std::vector<uint32_t> t((size_t)3 * OH_GRAIN_ENTRIES, 0);
    int planes = 0;
    for (int c = 0; c < 3; c++) {
        if (!sei->comp_model_present[c])
            continue;
        planes |= 1 << c;
        const int ni = sei->num_intensity_intervals_minus1[c] + 1, nv = sei->num_model_values_minus1[c] + 1;
        if (ni < 1 || ni > OH_FG_MAX_INTERVALS || nv < 1 || nv > 3)
            return OH_E_UNSUPPORTED;
        bool covered[OH_GRAIN_ENTRIES] = {};
        for (int i = 0; i < ni; i++) {
            const int32_t *v = sei->value[c][i];
            const int32_t sigma = v[0], fh = nv > 1 ? v[1] : 8, fv = nv > 2 ? v[2] : fh;
            if (sigma < 0 || sigma > 255 || !cut_ok(fh) || !cut_ok(fv) || sei->lower[c][i] > sei->upper[c][i])
                return OH_E_UNSUPPORTED;
            for (int a = sei->lower[c][i]; a <= sei->upper[c][i]; a++) {
                if (covered[a])
                    return OH_E_UNSUPPORTED;
                covered[a] = true;
                t[(size_t)c * OH_GRAIN_ENTRIES + a] = (uint32_t)sigma | (uint32_t)fh << 8 | (uint32_t)fv << 12;
            }
        }
    }
    memcpy(tables, t.data(), t.size() * sizeof(uint32_t));
    out->planes = planes; out->blending = sei->blending_mode_id; out->log2_scale = sei->log2_scale_factor;
    for (int c = 0; c < 3; c++)
        out->table[c] = tables[c];
    return OH_OK;
}

extern "C" int oh_grain_block(uint32_t seed, int c, int bx, int by, int *ox, int *oy, int *negate)
{
    if (!ox || !oy || !negate || c < 0 || c > 2 || bx < 0 || bx > 65535 || by < 0 || by > 65535)
        return OH_E_ARG;
    grain_block(seed, c, bx, by, ox, oy, negate);
    return OH_OK;
}

extern "C" int32_t oh_grain_mean(uint32_t sum, int n, int bit_depth)
{
    if ((n != 64 && n != 32 && n != 16) || !depth_ok(bit_depth))
        return -1;
    return grain_mean(sum, n, bit_depth);
}

/* the three below answer 0 outside their domains: nothing is shifted by an amount, and no product formed, that the kernel never sees */
static bool grain_in(int32_t g) { return g >= -OH_GRAIN_MAX && g <= OH_GRAIN_MAX; }

extern "C" int32_t oh_grain_value(int32_t sigma, int32_t p, int bit_depth, int log2_scale)
{
    if (sigma < 0 || sigma > 255 || p < -127 || p > 127 || !depth_ok(bit_depth) || log2_scale < 0 || log2_scale > 15)
        return 0;
    return grain_value(sigma, p, bit_depth, log2_scale);
}

extern "C" int32_t oh_grain_smooth(int32_t left, int32_t g, int32_t right)
{
    if (!grain_in(left) || !grain_in(g) || !grain_in(right))
        return 0;
    return grain_smooth(left, g, right);
}

extern "C" int32_t oh_grain_blend(int32_t s, int32_t g, int bit_depth, int blending)
{
    if (!depth_ok(bit_depth) || blending < 0 || blending > 1 || s < 0 || s >= 1 << bit_depth || !grain_in(g))
        return 0;
    return grain_blend(s, g, bit_depth, blending);
}

/* what oh_pics_grain checks of the OhGrain itself, for pictures of np planes */
int grain_check(const OhGrain *g, int np, std::string *why)
{
    char buf[256];
    if (g->planes < 0 || g->planes > 7) { snprintf(buf, sizeof(buf), "planes %d outside 0 .. 7", g->planes); *why = buf; return OH_E_ARG; }
    if (g->blending < 0 || g->blending > 1) { snprintf(buf, sizeof(buf), "blending %d outside 0 .. 1", g->blending); *why = buf; return OH_E_ARG; }
    if (g->log2_scale < 0 || g->log2_scale > 15) { snprintf(buf, sizeof(buf), "log2_scale %d outside 0 .. 15", g->log2_scale); *why = buf; return OH_E_ARG; }
    for (int c = 0; c < np; c++) {
        if (!(g->planes >> c & 1))
            continue;
        if (!g->table[c]) { snprintf(buf, sizeof(buf), "no table for plane %d", c); *why = buf; return OH_E_ARG; }
        for (int a = 0; a < OH_GRAIN_ENTRIES; a++) {
            const uint32_t t = g->table[c][a];
            if (t >> 16 || ((t & 255) && (!cut_ok((int)(t >> 8 & 15)) || !cut_ok((int)(t >> 12 & 15))))) {
                snprintf(buf, sizeof(buf), "table[%d][%d] = 0x%x: sigma | fh << 8 | fv << 12 with cut-offs 2 .. 14", c, a, t); *why = buf; return OH_E_ARG;
            }
        }
    }
    return OH_OK;
}

/* ---------------- colour remapping (remap.hip): the host-only helpers and what oh_pics_colour_remap checks ---------------- */
extern "C" int oh_remap_curve(int in_bit_depth, int out_bit_depth, int n, const uint16_t *coded, const uint16_t *target, uint16_t *out)
{
    if (!out || !depth_ok(in_bit_depth) || !depth_ok(out_bit_depth) || n < 0 || n > 33 || (n && (!coded || !target)))
        return OH_E_ARG;
    const int32_t Mi = (1 << in_bit_depth) - 1, Mo = (1 << out_bit_depth) - 1;
    int32_t x[35], y[35];
    int np = 0;
    if (!n || coded[0] > 0) { x[np] = 0; y[np++] = 0; }
    for (int k = 0; k < n; k++) {
        if (coded[k] > Mi || target[k] > Mo || (k && coded[k] <= coded[k - 1]))
            return OH_E_ARG;
        x[np] = coded[k]; y[np++] = target[k];
    }
    if (x[np - 1] < Mi) { x[np] = Mi; y[np++] = Mo; }
    out[x[0]] = (uint16_t)y[0];
    for (int k = 0; k + 1 < np; k++) {
        const int32_t dx = x[k + 1] - x[k];                     /* y (dx - t) + y' t + dx / 2 <= 4095 * 4095 + 2047 */
        for (int32_t t = 1; t <= dx; t++)
            out[x[k] + t] = (uint16_t)((y[k] * (dx - t) + y[k + 1] * t + (dx >> 1)) / dx);
    }
    return OH_OK;
}

/* what oh_pics_colour_remap checks of the OhRemap itself */
int remap_check(const OhRemap *r, std::string *why)
{
    char buf[256];
    if (!depth_ok(r->in_bit_depth) || !depth_ok(r->out_bit_depth)) {
        snprintf(buf, sizeof(buf), "bit depths %d -> %d: each 8, 9, 10 or 12", r->in_bit_depth, r->out_bit_depth); *why = buf; return OH_E_ARG;
    }
    if (r->log2_denom < 0 || r->log2_denom > REMAP_DENOM_MAX) {
        snprintf(buf, sizeof(buf), "log2_denom %d outside 0 .. %d", r->log2_denom, REMAP_DENOM_MAX); *why = buf; return OH_E_ARG;
    }
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 3; i++)
            if (r->coeff[c][i] < REMAP_COEFF_MIN || r->coeff[c][i] > REMAP_COEFF_MAX) {
                snprintf(buf, sizeof(buf), "coeff[%d][%d] = %d outside %d .. %d", c, i, r->coeff[c][i], REMAP_COEFF_MIN, REMAP_COEFF_MAX);
                *why = buf; return OH_E_ARG;
            }
    for (int k = 0; k < 6; k++) {
        const uint16_t *t = k < 3 ? r->pre[k] : r->post[k - 3];
        const int entries = 1 << (k < 3 ? r->in_bit_depth : r->out_bit_depth);
        if (!t) { snprintf(buf, sizeof(buf), "no %s table for component %d", k < 3 ? "pre" : "post", k % 3); *why = buf; return OH_E_ARG; }
        uint32_t top = 0;
        for (int v = 0; v < entries; v++)
            top = std::max<uint32_t>(top, t[v]);
        if (top >> r->out_bit_depth) {
            snprintf(buf, sizeof(buf), "%s[%d] holds %u, which does not fit %d bits", k < 3 ? "pre" : "post", k % 3, top, r->out_bit_depth);
            *why = buf; return OH_E_ARG;
        }
    }
    return OH_OK;
}

/* the matrix leaves the pre-table values as they are */
bool remap_is_identity(const OhRemap *r)
{
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 3; i++)
            if (r->coeff[c][i] != (c == i ? 1 << r->log2_denom : 0))
                return false;
    return true;
}

extern "C" int oh_remap_sample(const OhRemap *r, const uint16_t s[3], uint16_t out[3])
{
    std::string why;
    if (!r || !s || !out || remap_check(r, &why))
        return 0;
    const uint32_t in[3] = { s[0], s[1], s[2] };
    uint32_t o[3];
    remap_sample<false>(r->pre[0], r->pre[1], r->pre[2], r->post[0], r->post[1], r->post[2], &r->coeff[0][0], r->log2_denom,
                        (1u << r->in_bit_depth) - 1, (1 << r->out_bit_depth) - 1, in, o);
    for (int c = 0; c < 3; c++)
        out[c] = (uint16_t)o[c];
    return 1;
}

extern "C" int oh_remap_from_sei(const OhColourRemapSei *sei, uint16_t tables[6][4096], OhRemap *out)
{
    if (!sei || !tables || !out || !sei->present || sei->cancel)
        return OH_E_ARG;
    const int bi = sei->input_bit_depth, bo = sei->output_bit_depth;
    if (!depth_ok(bi) || !depth_ok(bo))
        return OH_E_UNSUPPORTED;
    std::vector<uint16_t> t((size_t)6 * 4096, 0);
    for (int c = 0; c < 3; c++) {
        const int npre = sei->pre_lut_num_val_minus1[c], npost = sei->post_lut_num_val_minus1[c];
        if (npre < 0 || npre >= OH_CRI_MAX_PIVOTS || npost < 0 || npost >= OH_CRI_MAX_PIVOTS)
            return OH_E_ARG;
        if (oh_remap_curve(bi, bo, npre ? npre + 1 : 0, sei->pre_lut_coded_value[c], sei->pre_lut_target_value[c], &t[(size_t)c * 4096]) ||
            oh_remap_curve(bo, bo, npost ? npost + 1 : 0, sei->post_lut_coded_value[c], sei->post_lut_target_value[c], &t[(size_t)(3 + c) * 4096]))
            return OH_E_ARG;
    }
    memcpy(tables, t.data(), t.size() * sizeof(uint16_t));
    out->in_bit_depth = bi; out->out_bit_depth = bo;
    out->log2_denom = sei->matrix_present ? sei->log2_matrix_denom : 0;
    for (int c = 0; c < 3; c++) {
        for (int i = 0; i < 3; i++)
            out->coeff[c][i] = sei->matrix_present ? sei->coeffs[c][i] : c == i;
        out->pre[c] = tables[c]; out->post[c] = tables[3 + c];
    }
    return OH_OK;
}

extern "C" int oh_remap_luts(const OhRemap *r, uint16_t out[3][4096])
{
    std::string why;
    if (!r || !out || remap_check(r, &why))
        return OH_E_ARG;
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 3; i++)
            if (c != i && r->coeff[c][i])
                return OH_E_UNSUPPORTED;
    const int32_t Mo = (1 << r->out_bit_depth) - 1;
    for (int c = 0; c < 3; c++) {
        int32_t k[3] = { 0, 0, 0 };
        k[c] = r->coeff[c][c];
        for (int v = 0; v < 1 << r->in_bit_depth; v++) {
            const int32_t p = r->pre[c][v];
            out[c][v] = r->post[c][remap_row(k, p, p, p, r->log2_denom, Mo)];
        }
    }
    return OH_OK;
}

/* ---------------- frame packing (packing.hip): the host-only helpers and what oh_pics_unpack / oh_pics_pack check ---------------- */
extern "C" int oh_packing_from_sei(const OhFramePackingSei *sei, OhPacking *out)
{
    if (!sei || !out || !sei->present || sei->cancel)
        return OH_E_ARG;
    if (sei->arrangement_type != OH_PACK_SIDE_BY_SIDE && sei->arrangement_type != OH_PACK_TOP_BOTTOM)
        return OH_E_UNSUPPORTED;                                /* 5: nothing to unpack; the others: not defined by HEVC */
    if (sei->field_views)
        return OH_E_UNSUPPORTED;
    OhPacking pk;
    memset(&pk, 0, sizeof(pk));
    pk.arrangement = sei->arrangement_type;
    pk.quincunx = sei->quincunx_sampling != 0;
    pk.flip[0] = sei->spatial_flipping && sei->frame0_flipped;
    pk.flip[1] = sei->spatial_flipping && !sei->frame0_flipped;
    pk.grid_x[0] = sei->frame0_grid_position_x; pk.grid_y[0] = sei->frame0_grid_position_y;
    pk.grid_x[1] = sei->frame1_grid_position_x; pk.grid_y[1] = sei->frame1_grid_position_y;
    pk.content_interpretation = sei->content_interpretation_type;
    std::string why;
    if (packing_check(&pk, &why))
        return OH_E_ARG;
    *out = pk;
    return OH_OK;
}

extern "C" const char *oh_packing_unsupported(const OhFramePackingSei *sei)
{
    if (!sei || !sei->present || sei->cancel)
        return "";
    if (sei->arrangement_type == 5)
        return "temporal interleaving: there is nothing to unpack, current_frame_is_frame0_flag says which view a picture is";
    if (sei->arrangement_type != OH_PACK_SIDE_BY_SIDE && sei->arrangement_type != OH_PACK_TOP_BOTTOM)
        return "an arrangement type that HEVC does not define (3 side by side, 4 top-bottom, 5 temporal interleaving)";
    if (sei->field_views)
        return "field_views_flag: the views as fields of one frame are not unpacked";
    return "";
}

/* what oh_pics_unpack / oh_pics_pack check of the OhPacking itself */
int packing_check(const OhPacking *pk, std::string *why)
{
    char buf[256];
    if (pk->arrangement != OH_PACK_SIDE_BY_SIDE && pk->arrangement != OH_PACK_TOP_BOTTOM) {
        snprintf(buf, sizeof(buf), "arrangement %d (3 side by side, 4 top-bottom)", pk->arrangement); *why = buf; return OH_E_ARG;
    }
    if ((pk->quincunx | pk->flip[0] | pk->flip[1]) & ~1) {
        snprintf(buf, sizeof(buf), "quincunx %d, flip %d / %d (0 or 1)", pk->quincunx, pk->flip[0], pk->flip[1]); *why = buf; return OH_E_ARG;
    }
    for (int v = 0; v < 2; v++)
        if ((pk->grid_x[v] | pk->grid_y[v]) & ~15) {
            snprintf(buf, sizeof(buf), "grid position (%d, %d) of frame %d (0 .. 15)", pk->grid_x[v], pk->grid_y[v], v); *why = buf; return OH_E_ARG;
        }
    return OH_OK;
}

/* the plane classes of a call on packed pictures of params `packed` with views of half or full size, and (view non-null) the params of
 * such a view: the packed pictures' with the view's size, each side rounded up to the minimum coding block */
int packing_geometry(const OhPacking *pk, const OhPicParams *packed, int full, PkPlane pl[2], OhPicParams *view, std::string *why)
{
    char buf[256];
    if (const int rc = packing_check(pk, why))
        return rc;
    const bool sbs = pk->arrangement == OH_PACK_SIDE_BY_SIDE;
    const int W = packed->width, H = packed->height, hs = oh_hshift(packed, 1), vs = oh_vshift(packed, 1);
    if (W < 1 || H < 1 || (sbs ? W % (2 << hs) : H % (2 << vs))) {
        snprintf(buf, sizeof(buf), "packed pictures of %dx%d: each half is a whole number of chroma samples, the %s a multiple of %d", W, H,
                 sbs ? "width" : "height", sbs ? 2 << hs : 2 << vs);
        *why = buf; return OH_E_ARG;
    }
    for (int q = 0; q < 2; q++) {
        const int qs = q ? hs : 0, qv = q ? vs : 0;
        PkPlane &p = pl[q];
        p.sbs = sbs; p.quincunx = pk->quincunx; p.full = full != 0; p.taps = q ? 4 : 8;
        p.pos = sbs ? (qs ? PK_POS_COSITED : PK_POS_PLAIN) : (qv ? PK_POS_MIDWAY : PK_POS_PLAIN);
        p.cw = (W >> qs) / (sbs ? 2 : 1); p.ch = (H >> qv) / (sbs ? 1 : 2);
        p.vw = full ? W >> qs : p.cw; p.vh = full ? H >> qv : p.ch;
        p.maxv = (1 << packed->bit_depth) - 1;
    }
    if (view) {
        const int cb = 1 << packed->log2_min_cb_size;
        *view = *packed;
        view->width = (pl[0].vw + cb - 1) / cb * cb;
        view->height = (pl[0].vh + cb - 1) / cb * cb;
    }
    return OH_OK;
}

extern "C" int oh_packing_view_size(const OhPacking *pk, const OhPicParams *packed, int full, OhPicParams *view)
{
    if (!pk || !packed || !view || (full & ~1) || packed->log2_min_cb_size < 3 || packed->log2_min_cb_size > 6 || !depth_ok(packed->bit_depth) ||
        packed->chroma_format_idc < 0 || packed->chroma_format_idc > 3)
        return OH_E_ARG;
    PkPlane pl[2];
    OhPicParams v;
    std::string why;
    if (const int rc = packing_geometry(pk, packed, full, pl, &v, &why))
        return rc;
    *view = v;
    return OH_OK;
}

extern "C" int oh_packing_views(const OhPacking *pk, int *left, int *right)
{
    if (!pk || !left || !right)
        return 0;
    if (pk->content_interpretation != 1 && pk->content_interpretation != 2)
        return 0;
    *left = pk->content_interpretation == 1 ? 0 : 1;
    *right = 1 - *left;
    return 1;
}

template <typename T>
static int packing_sample_t(const PkPlane &pl, int v, int flip, int g, int x, int y, const T *plane, ptrdiff_t stride)
{
    const T *r = plane + (pl.sbs ? (ptrdiff_t)v * pl.cw : (ptrdiff_t)v * pl.ch * stride);
    return pk_unpack_sample(pl, v, flip, g, x, y, [=](int ry, int rx) -> int { return r[(ptrdiff_t)ry * stride + rx]; });
}

extern "C" int oh_packing_sample(const OhPacking *pk, const OhPicParams *packed, int full, int view, int plane, int x, int y,
                                 const void *samples, int stride, int32_t *out)
{
    OhPicParams vp;
    if (!samples || !out || (view & ~1) || plane < 0 || plane > 2 || oh_packing_view_size(pk, packed, full, &vp))
        return OH_E_ARG;
    if (plane && !packed->chroma_format_idc)
        return OH_E_ARG;
    PkPlane pl[2];
    std::string why;
    if (packing_geometry(pk, packed, full, pl, nullptr, &why))
        return OH_E_ARG;
    const int q = plane ? 1 : 0;
    if (x < 0 || y < 0 || x >= vp.width >> oh_hshift(&vp, q) || y >= vp.height >> oh_vshift(&vp, q) || stride < packed->width >> oh_hshift(packed, q))
        return OH_E_ARG;
    const bool sbs = pk->arrangement == OH_PACK_SIDE_BY_SIDE;
    const int flip = pk->flip[view], g = sbs ? pk->grid_x[view] : pk->grid_y[view];
    *out = packed->bit_depth == 8 ? packing_sample_t(pl[q], view, flip, g, x, y, (const uint8_t *)samples, stride)
                                  : packing_sample_t(pl[q], view, flip, g, x, y, (const uint16_t *)samples, stride);
    return OH_OK;
}

extern "C" int oh_packing_pack_sample(const OhPacking *pk, const OhPicParams *packed, int plane, int x, int y, const void *view0,
                                      const void *view1, int stride, int32_t *out)
{
    OhPicParams vp;
    if (!view0 || !view1 || !out || plane < 0 || plane > 2 || !pk || oh_packing_view_size(pk, packed, pk->quincunx, &vp))
        return OH_E_ARG;
    if (plane && !packed->chroma_format_idc)
        return OH_E_ARG;
    PkPlane pl[2];
    std::string why;
    if (packing_geometry(pk, packed, pk->quincunx, pl, nullptr, &why))
        return OH_E_ARG;
    const int q = plane ? 1 : 0;
    if (x < 0 || y < 0 || x >= packed->width >> oh_hshift(packed, q) || y >= packed->height >> oh_vshift(packed, q) || stride < pl[q].vw)
        return OH_E_ARG;
    const void *const views[2] = { view0, view1 };
    const bool b8 = packed->bit_depth == 8;
    *out = pk_pack_sample(pl[q], pk->flip, x, y, [=](int v, int sy, int sx) -> int {
        const ptrdiff_t at = (ptrdiff_t)sy * stride + sx;
        return b8 ? ((const uint8_t *)views[v])[at] : ((const uint16_t *)views[v])[at];
    });
    return OH_OK;
}
