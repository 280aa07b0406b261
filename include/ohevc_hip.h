/*
 * ohevc_hip.h — C ABI of the MI355X block-reconstruction engine (libohevc_hip.so).
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.  The engine owns
 * the decoded pictures in HBM (the DPB lives on the GPU), replays recorded work lists
 * (ohevc_frame.h) as whole-picture passes and hands pictures back on request:
 *
 *   reference side (kept intact)                       engine entry point
 *   ------------------------------------------------   -----------------------------------------
 *   set_sps -> ff_hevc_dsp_init/ff_hevc_pred_init       oh_engine_create        hevc.c:421-423
 *   ff_hevc_set_new_ref -> ff_thread_get_buffer         oh_pic_alloc            hevc_refs.c:75-147
 *   hls_slice_data end / frame done                     oh_frame_submit         hevc.c:3017-3090
 *   libOpenHevcDecode before exposing a picture         oh_engine_sync          openHevcWrapper.c:130-153
 *   libOpenHevcGetOutput(Cpy), calc_md5                 oh_pic_download         openHevcWrapper.c:338-398, hevc.c:4146-4169
 *   ff_hevc_output_frame crop + GetOutputCpy            oh_pic_download_window  hevc_refs.c:248-254, openHevcWrapper.c:353-398
 *   ff_hevc_unref_frame                                 oh_pic_free             hevc_refs.c:45-65
 *
 * All functions return 0 on success and a negative OH_E_* code otherwise; the table slots of the
 * reference cannot fail (void returns), so recording never reports errors —
 * they surface here, at submit / sync.  There is NO CPU fallback: every entry point fails with
 * OH_E_HIP when no gfx950 device is usable.
 *
 * Threading: an engine is a single-submitter object (one HIP stream, one picture table); calls on the same engine
 * must be serialised by the caller (the reference's frame threads each record into their own OhRecorder and hand the
 * finished work list to the thread that owns the engine).  Different engines are independent.
 */
#ifndef OHEVC_HIP_H
#define OHEVC_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "ohevc_frame.h"
#include "ohevc_annexb.h"                  /* OhPictureHash */

#ifdef __cplusplus
extern "C" {
#endif

enum {
    OH_OK = 0,
    OH_E_HIP = -1,        /* HIP runtime error (see oh_engine_last_error) */
    OH_E_ARG = -2,        /* invalid argument / inconsistent work list    */
    OH_E_NOMEM = -3,
    OH_E_UNSUPPORTED = -4 /* outside what the path covers (e.g. up-sampling of >8-bit pictures) */
};

enum OhPass {             /* indices into oh_engine_pass_times()          */
    OH_PASS_INTER = 0, OH_PASS_RESIDUAL, OH_PASS_INTRA, OH_PASS_DEBLOCK_V, OH_PASS_DEBLOCK_H,
    OH_PASS_SAO, OH_N_PASSES
};

typedef struct OhEngine   OhEngine;
typedef struct OhDevFrame OhDevFrame;

int  oh_engine_create(OhEngine **out, int device);
/* page-locked host memory: a work list whose arrays ALL lie in blocks from oh_host_alloc() may carry OH_FRAME_PINNED (ohevc_frame.h) and
 * is then copied to the GPU by DMA from where it lies (no staging copy on the host thread) */
void *oh_host_alloc(size_t bytes);
void  oh_host_free(void *p);
/* same, but every kernel and copy is enqueued on the caller's stream (hipStream_t passed as
 * void*; e.g. torch.cuda.current_stream().cuda_stream) so that RCCL collectives issued by the
 * caller on that stream are ordered with the engine's passes.  The stream is not destroyed. */
int  oh_engine_create_on_stream(OhEngine **out, int device, void *hip_stream);
void oh_engine_destroy(OhEngine *e);
const char *oh_engine_last_error(const OhEngine *e);
int  oh_engine_sync(OhEngine *e);                       /* wait for everything enqueued so far */

/* pictures (device resident).  ids are small integers, stable until oh_pic_free */
int oh_pic_alloc(OhEngine *e, const OhPicParams *p, int *pic_id);
int oh_pic_free(OhEngine *e, int pic_id);
/* A picture is two buffers of oh_pic_bytes()/2 bytes each: the reconstruction/deblock planes
 * ("half 0") and the SAO output planes ("half 1"); layout inside a half: oh_pic_half_layout().
 * oh_pic_wrap builds a picture over caller-owned device memory (two 256-byte aligned buffers, e.g.
 * rows of a torch uint8 tensor) so that finished reference pictures of several GPUs sit
 * contiguously and can be handed to one RCCL all-gather without a copy;
 * oh_pic_final_half tells which half holds the finished picture, oh_pic_set_final_half marks a
 * half as finished after the caller filled it (broadcast / all-gather receive side). */
size_t oh_pic_bytes(const OhPicParams *p);
int oh_pic_wrap(OhEngine *e, const OhPicParams *p, void *half0, void *half1, size_t half_bytes, int *pic_id);
int oh_pic_final_half(OhEngine *e, int pic_id);                 /* 0, 1 or a negative error */
int oh_pic_set_final_half(OhEngine *e, int pic_id, int half);
/* planes: tightly described by byte strides, sample type uint8_t (8 bit) or uint16_t (>8 bit) */
int oh_pic_upload(OhEngine *e, int pic_id, const uint8_t *const planes[3], const ptrdiff_t strides[3]);
int oh_pic_download(OhEngine *e, int pic_id, uint8_t *const planes[3], const ptrdiff_t strides[3]);

/* output side: the picture inside its conformance window, packed — what ff_hevc_output_frame's
 * plane-pointer offsets (hevc_refs.c:248-254) followed by libOpenHevcGetOutputCpy's row copies (openHevcWrapper.c:353-398)
 * hand to the application.  Plane c receives ((height - top - bottom) >> vshift) rows of ((width - left - right) >> hshift)
 * samples starting at (left >> hshift, top >> vshift); strides[] are the destination pitches in bytes (>= the row size).
 * The copy goes through a pinned staging buffer of the engine. */
typedef struct OhWindow { int32_t left, right, top, bottom; } OhWindow;     /* luma samples, as HEVCWindow after hevc_ps.c scaled it */
int oh_pic_download_window(OhEngine *e, int pic_id, const OhWindow *win, uint8_t *const planes[3], const ptrdiff_t strides[3]);
/* The same fetch in two halves, for a decoder whose threads share one engine behind a lock (an engine is driven by one thread at a
 * time): oh_pic_download_start — under that lock, microseconds — enqueues the device-to-host copies behind the batch that finished the
 * picture; oh_download_finish may then run on ANY thread WITHOUT the lock, while other threads hand pictures over: it waits for the
 * copies, moves the rows into the caller's planes (OHEVC_FETCH_THREADS copy helpers, default 3, plus the calling thread) and returns
 * the staging buffer.  Every started download must be finished (also to release it: planes = NULL gives OH_E_ARG after the wait).
 * With frame threads this takes the fetch of a released picture off the decoder's serial path (openHevcWrapper.c:338-398 is called
 * between two libOpenHevcDecode calls while the workers keep decoding). */
typedef struct OhDownload OhDownload;
int oh_pic_download_start(OhEngine *e, int pic_id, const OhWindow *win, OhDownload **out);
int oh_download_finish(OhEngine *e, OhDownload *d, uint8_t *const planes[3], const ptrdiff_t strides[3]);

/* MD5 of the three planes of n finished pictures computed on the GPU — the digests of the decoded-picture-hash SEI (hevc.c:4146-4162,
 * calc_md5 hevc.c:4623-4638: whole coded planes, rows packed, little-endian samples).  digests: n x 3 x 16 bytes.  Waits for the engine. */
int oh_pics_md5(OhEngine *e, const int *pic_ids, int n, uint8_t *digests);
/* hash_type 0 MD5 (what oh_pics_md5 computes), 1 CRC, 2 checksum (H.265 Annex D decoded picture hash) of the whole coded planes
 * of n finished pictures; out[i]: present = 1, hash_type, and the plane values (planes a monochrome picture lacks: 0), in the
 * layout oh_sei_picture_hash fills, so a check is a comparison.  Waits for the engine stream.  n == 0: OH_OK.
 * OH_E_ARG: an unknown picture or hash_type outside 0..2. */
int oh_pics_hash(OhEngine *e, const int *pic_ids, int n, int hash_type, OhPictureHash *out);

/* Output to the GPU's own consumers: n finished pictures, cropped to a window, as standard images in caller-owned DEVICE memory
 * (DESIGN.md §3b has the exact definitions, which the tests check bit for bit).
 *   OH_CONV_PLANAR      the packed Y plane, then Cb, then Cr (I420 / I422 / I444; 4:0:0 gives Y only)
 *   OH_CONV_SEMIPLANAR  the packed Y plane, then one interleaved CbCr plane (NV12 / NV16 / NV24; P010 / P210 / P410 above 8 bit)
 *   OH_CONV_RGB_PLANAR  3 x H x W;  OH_CONV_RGB  H x W x 3;  OH_CONV_RGBA  H x W x 4 (alpha at full scale)
 * sample: NATIVE (YUV only: the stored samples, u8 at 8 bit, u16 above — LSB-aligned planar, MSB-aligned semi-planar) or U8 for the
 * YUV formats; U8, U16, F16 or F32 for the RGB formats, which up-sample the chroma (0 nearest, 1 linear with chroma_sample_loc_type 0
 * siting) and apply the H.273 matrix in the given range with integer coefficients (oh_convert_coeffs).  The matrix is read by the RGB
 * formats only. */
enum { OH_CONV_PLANAR = 0, OH_CONV_SEMIPLANAR, OH_CONV_RGB_PLANAR, OH_CONV_RGB, OH_CONV_RGBA };
enum { OH_CONV_NATIVE = 0, OH_CONV_U8, OH_CONV_U16, OH_CONV_F16, OH_CONV_F32 };
enum { OH_CONV_MAX_PICS = 64,     /* pictures per launch; a call with more is split into several launches */
       OH_CONV_NCOEFFS = 9 };     /* oh_convert_coeffs: cy, crv, cgu, cgv, cbu, y offset, chroma mid, shift S, target depth D */
typedef struct OhConvert {
    int32_t format;               /* OH_CONV_PLANAR .. OH_CONV_RGBA */
    int32_t sample;               /* OH_CONV_NATIVE .. OH_CONV_F32 */
    int32_t matrix;               /* H.273 matrix_coefficients: 1 BT.709, 5 or 6 BT.601, 9 BT.2020 non-constant luminance */
    int32_t full_range;           /* video_full_range_flag */
    int32_t chroma_filter;        /* 0 nearest, 1 linear (chroma_sample_loc_type 0) */
    OhWindow win;                 /* conformance window, luma samples, as for oh_pic_download_window */
} OhConvert;
/* n finished pictures with identical OhPicParams -> n images in caller-owned device memory of the engine's device, image i at
 * dst + i * image_stride.  Reads each picture's finished half; enqueued on the engine stream behind the work that finished the
 * pictures, returns without waiting (a kernel failure latched earlier surfaces at the next sync).  n == 0: OH_OK.
 * OH_E_ARG, nothing written: an unknown picture, pictures whose params differ, an empty window or one whose offsets are not multiples
 * of SubWidthC / SubHeightC, image_stride < oh_convert_image_bytes, image_stride or dst not a multiple of the output sample size,
 * (n - 1) * image_stride + image bytes > dst_bytes, a dst that is not device memory of the engine's device (or whose allocation ends
 * before the last image).  OH_E_UNSUPPORTED: a sample type that does not fit the format, a matrix outside
 * {1, 5, 6, 9} (RGB formats), a semi-planar image of a 4:0:0 picture. */
int    oh_pics_convert(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, void *dst, size_t image_stride, size_t dst_bytes);
/* host only: bytes of one image; 0 when the combination is not valid (what oh_pics_convert would refuse for these params) */
size_t oh_convert_image_bytes(const OhPicParams *p, const OhConvert *cv);
/* host only: the integers the kernel uses for an RGB conversion of bit_depth-bit pictures, OH_CONV_NCOEFFS of them (n: room in out) */
int    oh_convert_coeffs(const OhConvert *cv, int bit_depth, int32_t *out, int n);

/* The inverse of oh_pics_convert: n images in caller-owned DEVICE memory, in exactly the layouts oh_pics_convert writes, become n
 * finished engine pictures without a host round trip (DESIGN.md §3g has the exact definitions, which the tests check bit for bit
 * against tests/import_model.py).  cv describes the images: format, sample type, matrix, range, the chroma siting the RGB formats are
 * sub-sampled with (chroma_filter 0: the co-sited pixel, 1: the 1-2-1 filter of chroma_sample_loc_type 0) and win, the window of the
 * destination pictures that an image fills; image i lies at src + i * image_stride and takes oh_convert_image_bytes(params of the
 * destinations, cv) bytes.  YUV images must have the pictures' chroma format: NATIVE planar samples are clamped to the bit depth,
 * NATIVE semi-planar ones shifted down from the MSB, U8 ones shifted up.  RGB images go through the H.273 forward matrix in int32
 * (oh_import_coeffs), F16 / F32 samples as clamp(v, 0, 1) at 16 bit.  The rest of the coded planes replicates the window's edges, so
 * the whole picture is defined.  Writes half 0 of every destination (oh_pic_wrap pictures too) and marks it finished; enqueued on the
 * engine stream, returns without waiting: src must stay valid until the stream has passed the call.  n == 0: OH_OK.  More than
 * OH_CONV_MAX_PICS images are split into several launches.
 * OH_E_ARG, nothing written: a null argument, an unknown picture, destinations whose params differ, a destination listed twice, an
 * empty window or one whose offsets are not multiples of SubWidthC / SubHeightC, image_stride < the image size, image_stride or src not
 * a multiple of the sample size, (n - 1) * image_stride + image bytes > src_bytes, a src that is not device memory of the engine's
 * device (or whose allocation ends before the last image).  OH_E_UNSUPPORTED: what oh_pics_convert refuses with that code. */
enum { OH_IMPORT_NCOEFFS = 13 };  /* oh_import_coeffs: ry gy by  ru gu bu  rv gv bv  y offset, chroma mid, shift S, input depth D */
int    oh_pics_import(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, const void *src, size_t image_stride, size_t src_bytes);
/* host only: the integers the kernel uses for an RGB image of cv->sample (D = 8 for U8, else 16) into bit_depth-bit pictures,
 * OH_IMPORT_NCOEFFS of them (n: room in out) */
int    oh_import_coeffs(const OhConvert *cv, int bit_depth, int32_t *out, int n);

/* Colour conversion on top of the RGB formats (DESIGN.md §3d has the exact definition, which the tests check bit for bit against
 * tests/colour_model.py): the non-linear R'G'B' of oh_pics_convert at 16 bit goes through the source's transfer curve to linear light,
 * one gain on a norm (the HLG OOTF and / or the BT.2390 tone curve), the primaries' 3 x 3 matrix with a clip, and the output curve —
 * every curve a table of integers built on the host (oh_colour_tables), the kernel all integer but for the one multiply of LINEAR. */
enum { OH_COL_LINEAR = 0, OH_COL_SRGB, OH_COL_GAMMA24 };      /* out_transfer */
enum { OH_TONE_NONE = 0, OH_TONE_BT2390 };
enum { OH_NORM_MAXRGB = 0, OH_NORM_LUMA };
enum { OH_COL_NA = 4097,          /* entries of the source-curve table A */
       OH_COL_NP = 1602,          /* entries of the piecewise-logarithmic tables G (gain) and B (output curve) */
       OH_COL_NMISC = 20 };       /* misc: M[3][3] Q20 (0..8), luminance weights Q14 (9..11), norm (12), output by table (13: 0 LINEAR),
                                     bits of the f32 K (14), gain stage active (15), matrix stage active (16), rest 0 */
typedef struct OhColour {
    int32_t in_transfer;          /* H.273: 16 PQ, 18 HLG, 13 sRGB, 1 / 6 / 14 / 15 SDR video (decoded with the BT.1886 display gamma 2.4) */
    int32_t in_primaries;         /* H.273: 1 BT.709, 9 BT.2020, 12 P3-D65 */
    int32_t out_primaries;
    int32_t out_transfer;         /* OH_COL_* */
    int32_t tone, norm;           /* OH_TONE_*, OH_NORM_* */
    float   src_peak;             /* nits: PQ mastering peak (read by the tone curve only), HLG nominal peak Lw, SDR / sRGB peak white */
    float   dst_peak;             /* nits at output code 1.0 (SRGB / GAMMA24) */
    float   white;                /* nits at output value 1.0 (LINEAR) */
} OhColour;
/* oh_pics_convert with the colour stages behind the matrix: everything oh_pics_convert says about pictures, windows, dst, strides,
 * ordering, n == 0 and splitting holds; image sizes are those of oh_convert_image_bytes.
 * OH_E_ARG, nothing written: a null col, an enum value (out_transfer, tone, norm) outside its list, a peak or white that is not finite
 * and positive.  OH_E_UNSUPPORTED: a YUV format; a transfer or primaries code outside the lists above; U8 or U16 samples with
 * OH_COL_LINEAR; HLG with OH_NORM_MAXRGB (its OOTF is defined on luminance) or with src_peak outside [400, 10000]; OH_TONE_BT2390
 * with dst_peak >= src_peak or with a knee at or below black (dst_peak below about a third of src_peak in the PQ domain); a table
 * whose neighbouring entries differ by more than its interpolation holds (2^19 or more between interpolated entries of G and B,
 * 2^24 or more or downwards in A). */
int    oh_pics_convert_colour(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, const OhColour *col, void *dst,
                              size_t image_stride, size_t dst_bytes);
/* host only: exactly the integers the kernel receives — A[OH_COL_NA], G[OH_COL_NP], B[OH_COL_NP], misc[OH_COL_NMISC] */
int    oh_colour_tables(const OhColour *col, int32_t *A, int32_t *G, int32_t *B, int32_t *misc);

/* Light-level statistics of finished pictures (DESIGN.md §3e has the exact definition, which the tests check bit for bit against
 * tests/light_model.py): what a caller needs to choose OhColour.src_peak from the pictures themselves, where the stream's MaxCLL is
 * absent or wrong.  Every pixel of the window goes through oh_pics_convert's chroma placement and 16-bit matrix (cv->matrix,
 * full_range, chroma_filter, win; cv->format and cv->sample are not read; a 4:0:0 picture has Cb = Cr = mid) and the source curve of
 * oh_pics_convert_colour to linear light l, 2^30 = full scale: 10000 nits for PQ, src_peak nits otherwise.  For HLG that is
 * SCENE-linear light, before the OOTF (full scale = the nominal peak's scene value 1).  The norm v of a pixel is max(lR, lG, lB)
 * (OH_NORM_MAXRGB) or its luminance (wR lR + wG lG + wB lB + 2^13) >> 14 (OH_NORM_LUMA).  The curve A and the weights are those of
 * oh_colour_tables (A, misc[9..11]) for { in_transfer, in_primaries, in_primaries, OH_COL_LINEAR, OH_TONE_NONE, OH_NORM_LUMA,
 * src_peak, 100, src_peak } (HLG: with 1000 for src_peak; neither depends on it).
 * The histogram has 16 bins per octave: bin 0 holds v < 2^14 (below 0.15 nits of PQ), bin 1 + 16 (e - 14) + ((v >> (e - 4)) & 15)
 * the v with floor(log2 v) = e in 14 .. 30; bin 257 is v = 2^30 alone. */
enum { OH_LL_NBINS = 258 };
typedef struct OhLightSpec {
    int32_t in_transfer;          /* H.273: 16 PQ, 18 HLG, 13 sRGB, 1 / 6 / 14 / 15 SDR video */
    int32_t in_primaries;         /* H.273: 1 BT.709, 9 BT.2020, 12 P3-D65 (the luminance weights of OH_NORM_LUMA) */
    int32_t norm;                 /* OH_NORM_MAXRGB, OH_NORM_LUMA */
    float   src_peak;             /* nits at full scale for every transfer except PQ */
} OhLightSpec;
typedef struct OhLightLevel {
    uint64_t pixels, sum;         /* pixels of the window; the sum of their v */
    uint32_t max, min;            /* of v */
    uint32_t hist[OH_LL_NBINS];   /* pixels per bin */
} OhLightLevel;
/* n finished pictures with identical OhPicParams -> out[0 .. n).  Reads each picture's finished half on the engine stream behind the
 * work that finished the pictures, waits for the stream like oh_pics_hash and fills out on the host; every call starts from zero.
 * More than OH_CONV_MAX_PICS pictures are split into several launches.  The results are exact integers and do not depend on the
 * order of accumulation.  n == 0: OH_OK.
 * OH_E_ARG, out untouched: a null cv, sp or out, an unknown picture, pictures whose params differ, an empty window or one whose offsets
 * are not multiples of SubWidthC / SubHeightC, a norm outside its list, a src_peak that is not finite and positive.
 * OH_E_UNSUPPORTED, out untouched: a transfer or primaries code outside the lists, a matrix outside {1, 5, 6, 9}, a table that
 * oh_colour_tables would refuse.  HLG takes either norm and any src_peak here (oh_pics_convert_colour restricts both for its OOTF). */
int      oh_pics_light_level(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, const OhLightSpec *sp, OhLightLevel *out);
/* host only: bin(v), v clamped to 2^30 */
int      oh_light_bin(uint32_t v);
/* host only: the largest v of a bin: 2^14 - 1 for bin 0, min(((17 + j) << (e - 4)) - 1, 2^30) for bin 1 + 16 (e - 14) + j; a bin
 * below 0 gives 0, one above 257 gives 2^30 */
uint32_t oh_light_bin_upper(int bin);
/* host only: the n pictures pooled as one scene.  b = the smallest bin whose cumulative count times 10^6 reaches ppm times the pixels
 * of all n (64-bit integers); *value = min(oh_light_bin_upper(b), the largest max of the n): at least ppm / 10^6
 * of the pixels are at or below *value.  OH_E_ARG: a null pointer, n < 1,
 * ppm > 10^6, no pixels. */
int      oh_light_percentile(const OhLightLevel *ll, int n, uint32_t ppm, uint32_t *value);

/* Resizing of finished pictures into engine pictures (DESIGN.md §3c has the exact definition, which the tests check bit for bit
 * against tests/resize_model.py): every plane is resampled on its own in integer arithmetic, separably, horizontal pass first, with
 * an anti-aliased triangle (BILINEAR) or Keys cubic a = -1/2 (BICUBIC) filter whose taps are re-normalised at the window's edges.
 * The chroma planes of 4:2:0 and 4:2:2 are co-sited with the even luma column (chroma_sample_loc_type 0), centred vertically. */
enum { OH_RESIZE_BILINEAR = 0, OH_RESIZE_BICUBIC };
enum { OH_RESIZE_MAX_PICS = 64,   /* pictures per launch set (fewer when the intermediate of 64 would pass 512 MiB); a call with more is split */
       OH_RESIZE_MAX_DOWN = 128,  /* largest source : destination ratio per axis */
       OH_RESIZE_MAX_UP = 16 };   /* largest destination : source ratio per axis */
typedef struct OhResize {
    int32_t  filter;              /* OH_RESIZE_BILINEAR, OH_RESIZE_BICUBIC */
    OhWindow win;                 /* source window, luma samples, rules as for oh_pics_convert */
    int32_t  width, height;       /* size of the resized image, luma samples, inside the destination pictures */
} OhResize;
/* n finished source pictures (identical params) -> n destination pictures (identical params, same bit depth and chroma format as the
 * sources).  The image takes the top-left width x height of each destination; the rest of its coded planes replicates the image's
 * last column and last row.  Reads each source's finished half, writes half 0 of each destination and marks it finished; enqueued on
 * the engine stream behind the work that finished the sources, returns without waiting.  n == 0: OH_OK.
 * OH_E_ARG, nothing written: unknown pictures; sources (or destinations) whose params differ among themselves; a picture that is both
 * source and destination, or a destination listed twice; an empty window or one whose offsets are not multiples of SubWidthC /
 * SubHeightC; width / height below 1, above the destination's coded size or not multiples of SubWidthC / SubHeightC; an unknown filter.
 * OH_E_UNSUPPORTED: destinations whose bit depth or chroma format differs from the sources'; a plane whose window extent is more
 * than OH_RESIZE_MAX_DOWN times, or less than 1 / OH_RESIZE_MAX_UP of, its image extent on either axis. */
int oh_pics_resize(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhResize *rs);
/* host only: the integers the kernels receive for one axis.  phase: 2 (samples centred in their cells) or 1 (co-sited chroma columns).
 * Output sample x uses n_taps[x] source samples from first[x] (an index inside the window) with coeffs[x * max_taps + 0 .. n_taps[x])
 * (the rest of the row is zero), which sum to 1 << 14.  OH_E_ARG: extents below 1 or above 16384, an unknown filter or phase, max_taps
 * below oh_resize_max_taps.  OH_E_UNSUPPORTED: some output's absolute coefficients sum to 1 << 15 or more (no such geometry is known). */
int oh_resize_taps(int src_extent, int dst_extent, int filter, int phase, int32_t *first, int16_t *coeffs, int max_taps, int *n_taps);
/* host only: the largest number of taps of an output sample of that axis (OH_E_ARG as above) */
int oh_resize_max_taps(int src_extent, int dst_extent, int filter);

/* Comparison of finished pictures (DESIGN.md §3f has the exact definition, which the tests check bit for bit against
 * tests/compare_model.py): per plane of a pair (a, b) the number of differing samples, sum |a - b|, sum (a - b)^2, max |a - b|, the
 * first differing sample in raster order, and SSIM over 8x8 windows at stride 4 as an exact integer sum of Q30 window values — what
 * PSNR and mean SSIM are made of, and the answer to "which plane, how many samples, where is the first one" behind a hash mismatch,
 * without a host copy of a picture.  Every field is an integer sum, count or extremum: the result does not depend on the order of
 * accumulation. */
enum { OH_CMP_SSIM = 1 };                     /* flags: also compute SSIM; without it the ssim_* fields are 0 */
enum { OH_CMP_NONE = 0xFFFFFFFFu };           /* first_x / first_y of a plane without a differing sample */
typedef struct OhCompareSpec {
    OhWindow win;                             /* luma samples, rules as for oh_pics_convert; plane c's window is it shifted by oh_hshift / oh_vshift */
    int32_t  flags;                           /* 0 or OH_CMP_SSIM */
} OhCompareSpec;
typedef struct OhPlaneDiff {
    uint64_t samples;                         /* samples of the plane's window */
    uint64_t differing;                       /* samples with a != b */
    uint64_t sad, sse;                        /* sum |a - b|, sum (a - b)^2 */
    uint32_t max_abs;                         /* max |a - b| */
    uint32_t first_x, first_y;                /* first differing sample in raster order, plane-window coordinates */
    uint64_t ssim_windows;                    /* 8x8 windows evaluated */
    int64_t  ssim_sum;                        /* sum over the windows of their SSIM in Q30 (signed) */
} OhPlaneDiff;
typedef struct OhCompare { OhPlaneDiff plane[3]; } OhCompare;   /* planes a 4:0:0 picture lacks: all zero, first_* = OH_CMP_NONE */
/* n pairs (a_ids[i], b_ids[i]) of finished pictures, all 2n with identical OhPicParams -> out[0 .. n).  Reads each picture's finished
 * half on the engine stream behind the work that finished the pictures, waits for the stream like oh_pics_light_level and fills out on
 * the host; every call starts from zero.  More than OH_CONV_MAX_PICS pairs are split into several launches.  A picture may appear in
 * many pairs and as both members of one; nothing is written to pictures.  n == 0: OH_OK.
 * OH_E_ARG, out untouched: a null sp, out or id array, an unknown picture, pictures whose params differ anywhere among the 2n (so
 * pictures of different bit depth, chroma format or size are an OH_E_ARG, never OH_E_UNSUPPORTED), an empty window or one whose offsets
 * are not multiples of SubWidthC / SubHeightC, flag bits other than OH_CMP_SSIM.  No combination gives OH_E_UNSUPPORTED. */
int     oh_pics_compare(OhEngine *e, const int *a_ids, const int *b_ids, int n, const OhCompareSpec *sp, OhCompare *out);
/* host only: c1 = (64 M^2 + 5000) / 10000 and c2 = (9 * 64 * 63 M^2 + 5000) / 10000 with M = 2^bit_depth - 1, in 64-bit integers (8 bit:
 * 416 and 235963).  OH_E_ARG: a null pointer, a bit depth outside 8 / 9 / 10 / 12. */
int     oh_compare_ssim_consts(int bit_depth, int64_t *c1, int64_t *c2);
/* host only: the Q30 value of one 8x8 window from its sums s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum ab — the very
 * function the kernel evaluates (csrc/compare_common.h).  A bit depth outside 8 / 9 / 10 / 12 gives 0. */
int64_t oh_compare_ssim_window(int bit_depth, uint32_t s1, uint32_t s2, uint64_t ss, uint64_t s12);
/* host only: 10 log10(M^2 samples / sse) in dB; +infinity for sse 0; NaN for samples 0 */
double  oh_compare_psnr(uint64_t sse, uint64_t samples, int bit_depth);

/* Composition of finished pictures (DESIGN.md §3h has the exact definition, which the tests check bit for bit against
 * tests/compose_model.py): n destination pictures are composed IN PLACE, on their finished halves — an optional fill of the whole coded
 * planes, then up to OH_COMPOSE_MAX_LAYERS layers in list order, each a rectangle of another finished picture placed at an offset,
 * with an opacity and an optional 8-bit alpha plane in caller-owned DEVICE memory, source over destination in code values with
 * straight alpha.  What a logo or burnt-in subtitles on every picture of a batch, picture-in-picture, a contact sheet and a letterbox
 * are made of: oh_pics_import turns an RGBA overlay into a picture (and leaves its alpha channel where it is, for this call),
 * oh_pics_resize scales it, this call puts it on.
 * Per sample of plane c: w = alpha * opacity (0 .. 65280; alpha 255 without a plane) and oh_compose_blend(dst, src, alpha, opacity) =
 * (src w + dst (65280 - w) + 32640) / 65280 in exact integers: w = 0 keeps dst, w = 65280 gives src.  Plane c of a layer is the rectangle,
 * the position and the clip shifted by oh_hshift / oh_vshift; the alpha of a chroma sample is oh_compose_chroma_alpha of the luma
 * alphas it covers (4:2:0 the rounded mean of 2 x 2, 4:2:2 of two, 4:4:4 the alpha itself). */
enum { OH_COMPOSE_MAX_LAYERS = 16 };
enum { OH_COMPOSE_FILL = 1 };                 /* flags */
typedef struct OhLayer {
    const int32_t *src_ids;       /* n finished pictures: the source of this layer for destination i (a logo: n times the same id) */
    int32_t  sx, sy, w, h;        /* rectangle of the source, luma samples: inside the source's coded size */
    int32_t  dx, dy;              /* where its top left goes in the destination, luma samples; may be negative or reach beyond: clipped */
    int32_t  opacity;             /* 0 .. 256 */
    const void *alpha;            /* NULL (255 everywhere) or DEVICE memory: one u8 per luma sample of the rectangle, straight (not premultiplied) */
    int64_t  alpha_pixel_stride, alpha_row_stride, alpha_image_stride;   /* bytes; image stride 0: all destinations share one plane */
} OhLayer;
typedef struct OhCompose {
    int32_t  flags;               /* 0 or OH_COMPOSE_FILL */
    int32_t  fill[3];             /* OH_COMPOSE_FILL: the Y, Cb, Cr sample values every coded plane starts from (4:0:0: fill[1..2] are not read) */
    int32_t  n_layers;            /* 0 .. OH_COMPOSE_MAX_LAYERS */
    const OhLayer *layers;        /* host array, applied in order */
} OhCompose;
/* n destinations with identical OhPicParams; the n pictures of one layer with identical params among themselves, of any size, but of
 * the destinations' bit depth and chroma format.  Reads each source's finished half and composes each destination's finished half (half
 * 0 of a picture nothing has finished yet): the whole coded planes with OH_COMPOSE_FILL — the old content is not read —, else the
 * bounding box of the layers clipped to the destination's coded size; which half is the finished one does not change.  A layer wholly
 * outside the destination changes nothing.  The luma alpha of rectangle sample (x, y) of destination i is the byte at alpha + i *
 * alpha_image_stride + y * alpha_row_stride + x * alpha_pixel_stride (pixel stride 4: the alpha channel of the RGBA image that went
 * into oh_pics_import); clipping moves the origin with the rectangle.  Enqueued on the engine stream behind the work that finished the
 * pictures, returns without waiting: the alpha planes must stay valid until the stream has passed the call.  n == 0: OH_OK.  More than
 * OH_CONV_MAX_PICS destinations are split into several launches.
 * OH_E_ARG, nothing written: a null e, cp or id array; n_layers outside 0 .. OH_COMPOSE_MAX_LAYERS, or null layers with n_layers > 0; an
 * unknown picture; destinations whose params differ, or the pictures of one layer whose params differ; a destination listed twice, or a
 * picture that is both a destination and a source; a source rectangle that is empty, not inside the source's coded size, or — like dx
 * and dy — not a multiple of SubWidthC / SubHeightC; an opacity outside 0 .. 256; flag bits other than OH_COMPOSE_FILL; a fill value
 * outside the bit depth; an alpha pointer that is not device memory of the engine's device, or whose allocation ends before the last
 * byte the unclipped rectangle of the last image addresses; negative alpha strides.
 * OH_E_UNSUPPORTED, nothing written: a layer whose pictures differ from the destinations in bit depth or chroma format. */
int      oh_pics_compose(OhEngine *e, const int *dst_ids, int n, const OhCompose *cp);
/* host only — the very functions the kernel evaluates (csrc/compose_common.h, shared by host and device like compare_common.h): the
 * blend of one sample of at most 12 bits (alpha 0 .. 255, opacity 0 .. 256), and the alpha of a chroma sample from the luma alphas
 * a00 a01 (upper luma row) and a10 a11 (lower) that it covers */
uint32_t oh_compose_blend(uint32_t dst, uint32_t src, uint32_t alpha, uint32_t opacity);
uint32_t oh_compose_chroma_alpha(int chroma_format_idc, uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11);

/* Reformatting of finished pictures (DESIGN.md §3j has the exact definition, which the tests check bit for bit against
 * tests/reformat_model.py): n finished pictures become n finished pictures of another bit depth (8 / 9 / 10 / 12) and / or another
 * chroma format (0 .. 3) and the same size — the call to make before oh_pics_resize, oh_pics_compose or oh_pics_compare when their
 * pictures are not of one kind.  Every destination sample is a weighted sum of source samples of its plane whose weights total 2^f
 * (f = 0: the sample itself), quantised ONCE by s = f + source depth - destination depth bits: oh_reformat_quantise.  Chroma that is
 * sub-sampled further takes the co-sited source sample (OH_RF_POINT) or the 1-2-1 filter across and the two rows down of
 * chroma_sample_loc_type 0 (OH_RF_LINEAR, the filter of oh_pics_import); chroma that is sub-sampled less takes the nearest source sample
 * (OH_RF_POINT) or the linear filter of oh_pics_convert (OH_RF_LINEAR).  A 4:0:0 destination gets no chroma; from a 4:0:0 source every
 * chroma sample is 2^(depth - 1).  The whole coded planes are converted, filter taps clamped at the edges of the coded source plane. */
enum { OH_RF_ROUND = 0, OH_RF_DITHER };          /* depth: round to nearest, or the ordered 4 x 4 dither */
enum { OH_RF_POINT = 0, OH_RF_LINEAR };          /* chroma_down, chroma_up (0 = point / nearest, 1 = linear, chroma_sample_loc_type 0) */
typedef struct OhReformat { int32_t depth, chroma_down, chroma_up; } OhReformat;
/* The n sources with identical OhPicParams, the n destinations with identical params, both of one width and height; bit depth and
 * chroma format may differ, the other fields are not compared.  Reads each source's finished half, writes half 0 of each destination and
 * marks it finished, like oh_pics_resize (pictures of oh_pic_wrap like allocated ones).  Enqueued on the engine stream behind the work
 * that finished the sources, returns without waiting.  The filter that matters is chosen by the direction of the change; the other
 * field is still checked.  Same depth and same format is a copy of the coded planes.  n == 0: OH_OK.  More than OH_CONV_MAX_PICS
 * pictures are split into several launches.
 * OH_E_ARG, nothing written: a null e, rf or id array; an unknown picture; sources (or destinations) whose params differ among
 * themselves; a width or height that differs between sources and destinations; a picture that is both source and destination, or a
 * destination listed twice; an enum value outside its list.  No combination gives OH_E_UNSUPPORTED. */
int     oh_pics_reformat(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhReformat *rf);
/* host only: the very function the kernel evaluates (csrc/reformat_common.h).  s <= 0: min(sum << -s, 2^bd - 1); s > 0:
 * min((sum + r) >> s, 2^bd - 1) with r = 2^(s - 1) (OH_RF_ROUND) or ((2 t + 1) << s) >> 5 (OH_RF_DITHER), t = B4[y & 3][x & 3],
 * B4 = {{0,8,2,10},{12,4,14,6},{3,11,1,9},{15,7,13,5}}; (x, y): the sample's place in its destination plane.  sum 0 .. 8 * 4095,
 * s -4 .. 7. */
int32_t oh_reformat_quantise(int32_t sum, int s, int depth_mode, int x, int y, int dst_bit_depth);

/* Orientation of finished pictures (DESIGN.md §3k has the exact definition, which the tests check bit for bit against
 * tests/orient_model.py): n finished pictures become n finished pictures that hold a window of them cropped, mirrored, turned by
 * quarter turns or transposed — what a display-orientation SEI (oh_sei_display_orientation, ohevc_annexb.h), the mirrored view of a
 * frame-packed pair or a portrait rendition asks for, without leaving YUV.  A permutation of stored samples.  Per plane c, S is the
 * plane's window: win shifted by oh_hshift / oh_vshift, Ws x Hs samples.
 *   1. OH_ORIENT_TRANSPOSE first:  T[y][x] = S[x][y] (Wt = Hs, Ht = Ws); without it T = S;
 *   2. OH_ORIENT_HFLIP next:       U[y][x] = T[y][Wt - 1 - x]; without it U = T;
 *   3. OH_ORIENT_VFLIP last:       I[y][x] = U[Ht - 1 - y][x]; without it I = U.
 * So 3 is a half turn, 5 (TRANSPOSE | HFLIP) a quarter turn clockwise, 6 (TRANSPOSE | VFLIP) a quarter turn anticlockwise and 7 the
 * anti-transpose.  The image I takes the top left of the destination plane; the rest of the destination's coded plane replicates I's
 * last column and last row, D[y][x] = I[min(y, Hi - 1)][min(x, Wi - 1)], as oh_pics_resize does, so the whole picture is defined and
 * hashes.  Samples are copied as stored: chroma is not re-filtered, so a mirrored 4:2:0 or 4:2:2 picture keeps its chroma samples and
 * their nominal siting moves by half a luma sample. */
enum { OH_ORIENT_HFLIP = 1, OH_ORIENT_VFLIP = 2, OH_ORIENT_TRANSPOSE = 4 };   /* orientation: any OR of these, 0 .. 7 */
typedef struct OhOrient {
    int32_t  orientation;   /* 0 .. 7 */
    OhWindow win;           /* source window, luma samples, rules as for oh_pics_convert */
} OhOrient;
/* The n sources with identical OhPicParams, the n destinations with identical params, of the sources' bit depth and chroma format and
 * of any size that holds the image.  Reads each source's finished half, writes half 0 of each destination and marks it finished, like
 * oh_pics_resize (pictures of oh_pic_wrap like allocated ones).  Enqueued on the engine stream behind the work that finished the
 * sources, returns without waiting.  n == 0: OH_OK.  More than OH_CONV_MAX_PICS pictures are split into several launches.
 * OH_E_ARG, nothing written: a null e, o or id array, or a negative n; an unknown picture; sources (or destinations) whose params
 * differ among themselves; a picture that is both source and destination, or a destination listed twice; an orientation outside
 * 0 .. 7; an empty window or one whose offsets are not multiples of SubWidthC / SubHeightC; an image (the window, its sides swapped
 * under OH_ORIENT_TRANSPOSE) wider or taller than the destination's coded size.
 * OH_E_UNSUPPORTED, nothing written: destinations of another bit depth or chroma format than the sources (oh_pics_reformat first);
 * OH_ORIENT_TRANSPOSE on 4:2:2 pictures, whose result would be 4:4:0 (reformat to 4:2:0 or 4:4:4 first).  Orientations 0 .. 3 are
 * fine on 4:2:2. */
int oh_pics_orient(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhOrient *o);
/* host only: the one orientation equal to applying `first`, then `second` (to the image of `first`); -1 outside 0 .. 7 */
int oh_orient_then(int first, int second);
/* host only: the orientation that undoes `orientation`: oh_orient_then(o, oh_orient_inverse(o)) == 0; -1 outside 0 .. 7 */
int oh_orient_inverse(int orientation);
/* host only: the size of the image of a w x h window: swapped under OH_ORIENT_TRANSPOSE.  OH_E_ARG: an orientation outside 0 .. 7, a
 * size below 1, a null pointer. */
int oh_orient_size(int orientation, int w, int h, int *ow, int *oh);
/* host only: the orientation that a display orientation SEI message recommends.  This comment is the contract: the message's flips
 * come first, then the anticlockwise rotation of the flipped picture, so the result is oh_orient_then((hor_flip ? 1 : 0) |
 * (ver_flip ? 2 : 0), R^k) with R = 6, a quarter turn anticlockwise, applied k = anticlockwise_rotation >> 14 times (the field counts
 * in units of 360 / 2^16 degrees).  OH_E_UNSUPPORTED: anticlockwise_rotation & 0x3FFF is not 0 — an angle that is no quarter turn
 * needs a resampler.  OH_E_ARG: a null pointer, a flag outside 0 / 1, a rotation of 2^16 or more. */
int oh_orient_from_sei(int hor_flip, int ver_flip, uint32_t anticlockwise_rotation, int *orientation);

/* Warping of finished pictures (DESIGN.md §3p has the exact definition, which the tests check bit for bit against
 * tests/warp_model.py): n finished pictures become n finished pictures resampled through one affine or perspective coordinate map —
 * rotation by any angle, shear, keystone correction, a stabilising shift, rotate-and-scale augmentation, the display-orientation SEI
 * at any angle — without leaving YUV.  Every sample is an exact integer.
 *
 * m is the INVERSE map, destination -> source, in luma samples: integer coordinates are sample positions, the top-left luma sample of
 * the source window is (0, 0) and so is the image's.
 *   m[0] m[1] m[3] m[4]   Q16, |.| <= 2^22          x_src = (m0 x + m1 y + m2) / W      W = 1 (affine)
 *   m[2] m[5]             Q16, |.| <= 2^36          y_src = (m3 x + m4 y + m5) / W      W = (m6 x + m7 y + m8) / 2^30 (perspective)
 *   m[6] m[7]             Q30 per sample, |.| <= 2^26
 *   m[8]                  Q30, 0 < m[8] <= 2^36; 2^30 when the map is affine
 * OH_WARP_AFFINE ignores m[6 .. 8].  Sample (x, y) of plane c of the image (shifts hs, vs; h = vs) has the luma position X = x << hs,
 * Y = y << vs and half a luma row more where vs = 1 (chroma_sample_loc_type 0, as in oh_pics_resize); in int64_t, >> flooring:
 *   Nx = m0 X + m1 Y + m2 + h (m1 >> 1),  Ny = m3 X + m4 Y + m5 + h (m4 >> 1),  D = m6 X + m7 Y + m8 + h (m7 >> 1)
 *   affine Lx = Nx; perspective Lx = floor(Nx 2^22 / (D >> 8)); Ly likewise; both clamped to [-2^30, 2^31 - 1]
 *   Px = Lx >> hs, Py = (Ly - vs 2^15) >> vs                                            the position in the plane's window, Q16
 *   NEAREST: ix = (Px + 2^15) >> 16;  else Qx = (Px + 512) >> 10, ix = Qx >> 6, fx = Qx & 63 (1/64 sample); y likewise.
 * A tap at plane index (i, j) of the plane's window of Wc x Hc samples: OH_WARP_REPLICATE clamps i to 0 .. Wc - 1 and j to
 * 0 .. Hc - 1; OH_WARP_CONSTANT gives fill[c] where i or j is outside.  Nothing outside the window is ever read.
 *   NEAREST   s(ix, iy)
 *   BILINEAR  t_j = (64 - fx) s(ix, j) + fx s(ix + 1, j), j = iy, iy + 1;  v = ((64 - fy) t_iy + fy t_(iy+1) + 2^11) >> 12
 *   BICUBIC   Keys, a = -1/2, 64 phases, taps c[f][0 .. 3] that sum to 1024 (oh_warp_cubic), at ix - 1 .. ix + 2, iy - 1 .. iy + 2:
 *             t_j = (sum_k c[fx][k] s(ix - 1 + k, j) + 8) >> 4;  v = clip((sum_j c[fy][j] t_j + 2^15) >> 16, 0, 2^bd - 1)
 * No anti-aliasing: a map that shrinks is point-sampled; oh_pics_resize is the call for scaling down.  The image takes the top left
 * width x height of each destination; the rest of the destination's coded planes replicates its last column and row. */
enum { OH_WARP_AFFINE = 0, OH_WARP_PERSPECTIVE };
enum { OH_WARP_NEAREST = 0, OH_WARP_BILINEAR, OH_WARP_BICUBIC };
enum { OH_WARP_REPLICATE = 0, OH_WARP_CONSTANT };
typedef struct OhWarp {
    int32_t  mode, filter, border;
    uint16_t fill[3];        /* code values per plane, OH_WARP_CONSTANT only */
    OhWindow win;            /* source window, luma samples, rules as for oh_pics_convert; nothing outside it is ever read */
    int32_t  width, height;  /* image size inside the destinations, luma samples */
    int64_t  m[9];           /* INVERSE map, destination -> source */
} OhWarp;
/* The n sources with identical OhPicParams, the n destinations with identical params, of the sources' bit depth and chroma format.
 * Reads each source's finished half, writes half 0 of each destination and marks it finished, like oh_pics_orient.  Enqueued on the
 * engine stream behind the work that finished the sources, returns without waiting.  n == 0: OH_OK after the OhWarp itself was
 * checked.  More than OH_CONV_MAX_PICS pictures are split into several launches.
 * OH_E_ARG, nothing written: a null e, w or id array, or a negative n; an unknown picture; sources (or destinations) whose params
 * differ among themselves; a picture that is both source and destination, or a destination listed twice; an empty window or one whose
 * offsets are not multiples of SubWidthC / SubHeightC; width or height below 1, above the destination's coded size or no multiple of
 * SubWidthC / SubHeightC; a mode, filter or border outside its list; with OH_WARP_CONSTANT a fill above the largest code value; a
 * coefficient outside the bounds above; OH_WARP_PERSPECTIVE with a denominator m6 x + m7 y + m8 below 2^20 at one of the four corner
 * samples of the image (it is linear, so the corners bound it).
 * OH_E_UNSUPPORTED, nothing written: destinations of another bit depth or chroma format than the sources (oh_pics_reformat first). */
int oh_pics_warp(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhWarp *w);
/* host only, exact integers, the very functions the kernel evaluates (csrc/warp_common.h).
 * oh_warp_position: the position (Q16, in the window of a plane with shifts hs, vs) that sample (x, y) of that plane of the image
 * reads; of w only mode and m are read.  OH_E_ARG: a null pointer, shifts outside 0 / 1, x or y negative or (x << hs, y << vs) above
 * 16384, a mode outside its list, a coefficient outside its bounds, a perspective denominator below 2^20 at the sample.
 * oh_warp_cubic: the four taps of phase f (0 .. 63); OH_E_ARG otherwise.
 * oh_warp_interp: one sample from its 4 x 4 neighbourhood, taps[4 j + i] = s(ix - 1 + i, iy - 1 + j) (NEAREST reads taps[5], BILINEAR
 * taps[5], [6], [9], [10]); -1: a null pointer, a fraction outside 0 .. 63, a filter outside its list, a depth that is not 8, 9, 10
 * or 12. */
int     oh_warp_position(const OhWarp *w, int hs, int vs, int x, int y, int32_t *px_q16, int32_t *py_q16);
int     oh_warp_cubic(int f, int16_t c[4]);
int32_t oh_warp_interp(const uint16_t taps[16], int fx, int fy, int filter, int bit_depth);
/* host only: how many workgroup tiles of a call with this OhWarp (mode, filter, width, height, m) into destinations of dst_width x
 * dst_height at this depth and chroma format stage their taps in LDS (*staged) and how many gather them from global memory
 * (*gathered): the kernel's own predicate, so that a test knows which paths it ran.  OH_E_ARG: what oh_pics_warp refuses of these. */
int     oh_warp_paths(const OhWarp *w, int bit_depth, int chroma_format_idc, int dst_width, int dst_height, int64_t *staged, int64_t *gathered);
/* host only, builders: each fills the whole OhWarp — OH_WARP_AFFINE, OH_WARP_BILINEAR, OH_WARP_REPLICATE, fill 0, the whole picture
 * as window, width = height = 0 (oh_warp_from_sei: the image size) — and the map.  OH_E_ARG: a null pointer, or as said.
 * oh_warp_translation: destination (x, y) reads source (x + dx_q2 / 4, y + dy_q2 / 4), the convention of OhMotionVector, so a global
 * vector of a motion field can be applied.
 * oh_warp_then: the one map equal to warping by `first`, then warping its image by `second` (affine maps only; m[6 .. 8] are not
 * read): A = A_first A_second with every product (a b + 2^15) >> 16; the result keeps first's filter, border, fill and window and
 * second's width and height.  OH_E_ARG also: a mode other than OH_WARP_AFFINE, a coefficient of an argument or of the result outside
 * its bounds.
 * oh_warp_invert: fwd as a source -> destination map becomes the destination -> source map (affine only), every term a quotient of
 * exact integers rounded to nearest (halves up) in __int128; the other fields are copied.  OH_E_ARG also: a singular map, a
 * coefficient of the argument or of the result outside its bounds.
 * oh_warp_rotation: an anticlockwise turn of the picture by `anticlockwise` (units of 360 / 2^16 degrees, below 2^16) that carries
 * the source position (cx_src, cy_src) to the destination position (cx_dst, cy_dst) (Q16, |.| <= 2^36): in y-down coordinates
 * x = x' cos - y' sin, y = x' sin + y' cos about the centres, times scale_q16 (1 .. 2^22: source samples per destination sample).
 * m0 = m4 = llrint(scale cos), m3 = -m1 = llrint(scale sin) with libm's cos / sin of a double — the only floating point of the
 * service — and exactly 0 / +-scale at multiples of a quarter turn; m2 = cx_src - ((m0 cx_dst + m1 cy_dst + 2^15) >> 16), m5 =
 * cy_src - ((m3 cx_dst + m4 cy_dst + 2^15) >> 16).  OH_E_ARG also: a result outside the bounds.
 * oh_warp_from_sei: the display-orientation SEI message at any angle for a picture of w x h luma samples (1 .. 16384): the flips come
 * first, then the anticlockwise rotation about the picture's centre, the order oh_orient_from_sei states.  The image is the rotated
 * bounding box, *ow = (|m0| w + |m1| h + 65535) >> 16 and *oh = (|m3| w + |m4| h + 65535) >> 16 of the rotation's terms, each rounded
 * up to a multiple of 2; the centres are (size - 1) << 15.  OH_E_ARG also: a flag outside 0 / 1, a rotation of 2^16 or more. */
int oh_warp_identity(OhWarp *out);
int oh_warp_translation(int32_t dx_q2, int32_t dy_q2, OhWarp *out);
int oh_warp_then(const OhWarp *first, const OhWarp *second, OhWarp *out);
int oh_warp_invert(const OhWarp *fwd, OhWarp *out);
int oh_warp_rotation(uint32_t anticlockwise, int64_t cx_src_q16, int64_t cy_src_q16, int64_t cx_dst_q16, int64_t cy_dst_q16, int32_t scale_q16,
                     OhWarp *out);
int oh_warp_from_sei(int hor_flip, int ver_flip, uint32_t anticlockwise_rotation, int w, int h, OhWarp *out, int *ow, int *oh);

/* Fields and frames (DESIGN.md §3l has the exact definitions, which the tests check bit for bit against tests/deinterlace_model.py).
 * The reference reads field_seq_flag and the pic_struct of the picture timing SEI (oh_sei_pic_timing, ohevc_annexb.h) and tags its
 * frames interlaced_frame / top_field_first; these calls act on it without a host copy.
 *
 * host only: what a pic_struct says (H.265 Table D.2).  This comment is the contract.
 *   kind          0 frame (pic_struct 0 and 3 .. 8), 1 top field (1, 9, 11), 2 bottom field (2, 10, 12);
 *   pair          -1 (9, 10): the field pairs with the previous picture in output order; +1 (11, 12): with the next; else 0;
 *   top_first     1 (3, 5), 0 (4, 6), -1 otherwise: which field of a frame is displayed first, where the message says so;
 *   repeat_first  1 (5, 6): the first field is shown again after the second; else 0;
 *   frames        2 (7, frame doubling), 3 (8, frame tripling), else 1.
 * OH_E_ARG: a null pointer, a pic_struct outside 0 .. 12. */
typedef struct OhFieldInfo { int32_t kind, pair, top_first, repeat_first, frames; } OhFieldInfo;
int oh_field_info(int pic_struct, OhFieldInfo *out);

/* n pairs of fields become n frames (weave), n frames become their fields (separate).  Per plane, over the whole coded planes:
 * D[2y][x] = T[y][x] and D[2y + 1][x] = B[y][x]; separate is the exact inverse.  Chroma planes follow the same row rule: an interlaced
 * 4:2:0 frame alternates its chroma rows by field too.  The 2n fields have identical OhPicParams; the n frames have identical params,
 * the fields' width, bit depth and chroma format and exactly twice their height; the other fields of the params are not compared
 * between fields and frames.  In oh_pics_separate one of top_ids / bottom_ids may be null: that field is not made.
 * Reads each source's finished half, writes half 0 of each destination and marks it finished, like oh_pics_orient (pictures of
 * oh_pic_wrap like allocated ones).  Enqueued on the engine stream behind the work that finished the sources, returns without waiting.
 * n == 0: OH_OK.  More than OH_CONV_MAX_PICS frames are split into several launches.
 * OH_E_ARG, nothing written: a null e or id array (but for the one of oh_pics_separate), or a negative n; both destination lists of
 * oh_pics_separate null; an unknown picture; fields (or frames) whose params differ among themselves; a width that differs between
 * fields and frames; a frame height that is not twice the field height; a picture that is both source and destination; a destination
 * listed twice, across both destination lists of oh_pics_separate.
 * OH_E_UNSUPPORTED, nothing written: a bit depth or chroma format that differs between fields and frames (oh_pics_reformat first);
 * this is looked at before the sizes. */
int oh_pics_weave(OhEngine *e, const int *top_ids, const int *bottom_ids, const int *dst_ids, int n);
int oh_pics_separate(OhEngine *e, const int *src_ids, const int *top_ids, const int *bottom_ids, int n);

/* Deinterlacing: n finished pictures (frames whose rows alternate between two fields) become n finished pictures of the same params.
 * The whole coded planes, every plane alike, no window (oh_pics_orient crops).  H x W is a plane's coded size (H is even), M =
 * 2^bit_depth - 1.  Rows with y % 2 == parity are the KEPT field, the others are MISSING.  Two row rules: clamped, r(k) = min(max(k, 0),
 * H - 1); mirrored, which always lands on a kept row: up = y - 1 >= 0 ? y - 1 : y + 1, dn = y + 1 <= H - 1 ? y + 1 : y - 1.  Columns
 * clamp: cx(k) = min(max(k, 0), W - 1).  C is the plane of cur.
 *   OH_DEINT_BOB       kept rows are copied; a missing row is (C[up][x] + C[dn][x] + 1) >> 1.  Reads nothing of the other field: called
 *                      twice, with parity 0 and 1, it gives field rate.
 *   OH_DEINT_BLEND     every row, kept or not: (C[r(y-1)][x] + 2 C[y][x] + C[r(y+1)][x] + 2) >> 2.  parity is checked, not used.
 *   OH_DEINT_LOWPASS5  kept rows are copied; a missing row is clip((-C[r(y-2)][x] + 4 C[r(y-1)][x] + 2 C[y][x] + 4 C[r(y+1)][x]
 *                      - C[r(y+2)][x] + 4) >> 3, 0, M), an arithmetic shift of the signed sum.  At 8 bit with parity 0 this is the
 *                      reference's deinterlace_bottom_field (imgconvert.c:299-379), whose edge rows are this clamping.
 *   OH_DEINT_ADAPTIVE  kept rows are copied; a missing row is motion-adaptive with an edge-directed spatial predictor.  P / C / N are
 *                      the planes of prev / cur / next; (A, B) = (P, C) when kept_first is 1 — the kept field is the earlier one of
 *                      its frame, so the other field's rows lie before it in prev and after it in cur — and (C, N) when it is 0.
 *                      All values signed 32 bit:
 *                          c = C[up][x]; e = C[dn][x]
 *                          t    = (A[y][x] + B[y][x]) >> 1
 *                          d0   = |A[y][x] - B[y][x]|
 *                          d1   = (|P[up][x] - c| + |P[dn][x] - e|) >> 1
 *                          d2   = (|N[up][x] - c| + |N[dn][x] - e|) >> 1
 *                          diff = max(d0 >> 1, d1, d2)
 *                          score(j) = sum over k in {-1, 0, 1} of |C[up][cx(x+k+j)] - C[dn][cx(x+k-j)]|
 *                          best = score(0) - 1; j* = 0
 *                          for s in (-1, +1), in this order:
 *                              if score(s) < best:   best = score(s); j* = s
 *                                  if score(2s) < best:   best = score(2s); j* = 2s      (tried only when s itself won)
 *                          sp  = (C[up][cx(x+j*)] + C[dn][cx(x-j*)]) >> 1
 *                          out = min(max(sp, t - diff), t + diff)
 *                      No clip is needed: sp and t lie in [0, M] and out lies between them.  With prev == cur == next the output is cur
 *                      exactly (diff == 0, t == C[y][x]): a still scene passes through untouched.
 * prev_ids / next_ids are read by OH_DEINT_ADAPTIVE only and not even checked by the other modes; a null array, or an entry of -1,
 * stands for the cur picture of that index (stream start and end).
 * All pictures involved have identical OhPicParams.  Reads finished halves, writes half 0 of each destination and marks it finished,
 * like oh_pics_orient; enqueued on the engine stream, returns without waiting.  n == 0: OH_OK.  More than OH_CONV_MAX_PICS pictures
 * are split into several launches.
 * OH_E_ARG, nothing written: a null e, d, cur_ids or dst_ids, or a negative n; an unknown picture, or an id below -1 in prev / next;
 * params that differ anywhere among cur, dst and (ADAPTIVE) prev / next — a bit depth or chroma format that differs is such a
 * difference, as in oh_pics_compare; a destination that is also any source of the call, or a destination listed twice; a mode outside
 * 0 .. 3; a parity or kept_first outside 0 / 1.  No combination gives OH_E_UNSUPPORTED. */
enum { OH_DEINT_BOB = 0, OH_DEINT_BLEND, OH_DEINT_LOWPASS5, OH_DEINT_ADAPTIVE };
typedef struct OhDeinterlace { int32_t mode, parity, kept_first; } OhDeinterlace;
int oh_pics_deinterlace(OhEngine *e, const int *prev_ids, const int *cur_ids, const int *next_ids,
                        const int *dst_ids, int n, const OhDeinterlace *d);
/* host only: the ADAPTIVE formula above on a window (the function the kernel evaluates, csrc/deinterlace_common.h): up[i] / dn[i] are
 * C[up][cx(x-3+i)] / C[dn][cx(x-3+i)]; a, b are A[y][x], B[y][x]; pu, pd, nu, nd are P[up][x], P[dn][x], N[up][x], N[dn][x]. */
int32_t oh_deint_adaptive(const int32_t up[7], const int32_t dn[7], int32_t a, int32_t b,
                          int32_t pu, int32_t pd, int32_t nu, int32_t nd);

/* Filters: n finished pictures become n finished pictures of the same params (the tests check every plane bit for bit
 * against tests/filter_model.py).  The whole coded planes, no window.  This comment is the contract.  H x W is a plane's coded size,
 * M = 2^bit_depth - 1; rows clamp, r(k) = min(max(k, 0), H - 1), and so do columns, cx(k) = min(max(k, 0), W - 1); S is the source
 * plane; q is 0 for luma and 1 for chroma; all arithmetic is signed 32 bit and >> is an arithmetic shift.
 * A tap set is LEGAL when nh and nv are odd and lie in 1 .. 15, the h and the v taps each sum to 256, and the sums of |h| and of |v|
 * are at most 512 each.  Then |tmp| <= 512 * 4095 and |acc| <= 512 * 512 * 4095 < 2^31 - 2^15: int32 never overflows at 12 bit.
 *   OH_FILTER_CONVOLVE  tmp[y][x] = sum over k of h[k] S[y][cx(x + k - nh / 2)], not rounded;
 *                       acc = sum over k of v[k] tmp[r(y + k - nv / 2)][x];
 *                       out = min(max((acc + 32768) >> 16, 0), M): one rounding per sample.  Taps {256} on both axes give a copy.
 *   OH_FILTER_UNSHARP   B is the CONVOLVE output of the plane with its class's taps, d = S - B; out = S where |d| <= threshold[q],
 *                       else min(max(S + ((amount[q] d + 32) >> 6), 0), M).  An amount of 64 adds the whole detail once, a negative
 *                       one softens, 0 is a copy.
 *   OH_FILTER_MEDIAN    the fifth smallest of the nine samples S[r(y + j)][cx(x + i)], i, j in {-1, 0, 1}.
 *   OH_FILTER_TEMPORAL  P / C / N are the planes of prev / src / next; mp = sum over i, j in {-1, 0, 1} of |P[r(y + j)][cx(x + i)] -
 *                       C[r(y + j)][cx(x + i)]|, mn the same with N; p' = mp <= threshold[q] ? P[y][x] : C[y][x], n' the same with
 *                       mn and N; out = (p' + 2 C[y][x] + n' + 2) >> 2.  With prev == src == next the output is src exactly; no clip
 *                       is needed.
 * planes: bit c set, plane c is filtered; clear, it is copied; bits of planes the format lacks are ignored.  taps[0] are luma's,
 * taps[1] those of both chroma planes; amount and threshold likewise.
 * prev_ids / next_ids are read by OH_FILTER_TEMPORAL only and not even checked by the other modes; a null array, or an entry of -1,
 * stands for the src picture of that index, as in oh_pics_deinterlace.
 * The fields a mode does not read are not checked: CONVOLVE ignores amount and threshold, MEDIAN and TEMPORAL ignore taps and amount
 * (MEDIAN the threshold too).  The fields it reads are checked for both classes, whatever `planes` says.
 * All pictures involved have identical OhPicParams.  Reads finished halves, writes half 0 of each destination and marks it finished,
 * like oh_pics_deinterlace; enqueued on the engine stream, returns without waiting.  n == 0: OH_OK (the OhFilter is checked all the
 * same, its thresholds against the M of 12 bit, there being no picture to take a depth from).  More than OH_CONV_MAX_PICS pictures are
 * split into several launches.
 * OH_E_ARG, nothing written: a null e, f, src_ids or dst_ids, or a negative n; an unknown picture, or an id below -1 in prev / next;
 * params that differ anywhere among src, dst and (TEMPORAL) prev / next; a destination that is also any source of the call, or a
 * destination listed twice; a mode outside 0 .. 3; planes outside 0 .. 7; illegal taps; an amount outside -64 .. 512; a threshold
 * outside 0 .. M (UNSHARP) or 0 .. 9 M (TEMPORAL).  No combination gives OH_E_UNSUPPORTED. */
enum { OH_FILTER_CONVOLVE = 0, OH_FILTER_UNSHARP, OH_FILTER_MEDIAN, OH_FILTER_TEMPORAL };
enum { OH_FILTER_MAX_TAPS = 15 };
typedef struct OhFilterTaps { int32_t nh, nv; int16_t h[OH_FILTER_MAX_TAPS], v[OH_FILTER_MAX_TAPS]; } OhFilterTaps;
typedef struct OhFilter {
    int32_t      mode;          /* OH_FILTER_* */
    int32_t      planes;        /* bit c set: plane c is filtered; clear: plane c is copied.  0 .. 7; bits of planes the format lacks are ignored */
    OhFilterTaps taps[2];       /* [0] luma, [1] both chroma planes: CONVOLVE, UNSHARP */
    int32_t      amount[2];     /* UNSHARP, in 1/64: -64 .. 512 */
    int32_t      threshold[2];  /* UNSHARP: 0 .. M;  TEMPORAL: 0 .. 9 * M */
} OhFilter;
int oh_pics_filter(OhEngine *e, const int *prev_ids, const int *src_ids, const int *next_ids,
                   const int *dst_ids, int n, const OhFilter *f);
/* host only: OH_OK for a legal tap set (above), else OH_E_ARG (a null pointer too) */
int oh_filter_taps_check(const OhFilterTaps *t);
/* host only: row n - 1 of Pascal's triangle scaled to sum 256, n in {1, 3, 5, 7, 9}: {256}, {64,128,64}, {16,64,96,64,16},
 * {4,24,60,80,60,24,4}, {1,8,28,56,70,56,28,8,1}; any other n, or a null pointer: OH_E_ARG */
int oh_filter_binomial(int n, int16_t *out);
/* host only: n equal taps, n odd in 1 .. 15: each 256 / n in integer division, the middle one the remainder more; else OH_E_ARG */
int oh_filter_box(int n, int16_t *out);
/* host only: the sample formulas above (the functions the kernel evaluates, csrc/filter_common.h).  oh_filter_unsharp: s the source
 * sample, b the CONVOLVE output; oh_filter_median9: the fifth smallest of nine values in any order; oh_filter_temporal: c / p / n the
 * samples of src / prev / next at one place, mp / mn the two window sums */
int32_t oh_filter_unsharp(int32_t s, int32_t b, int32_t amount, int32_t threshold, int32_t M);
int32_t oh_filter_median9(const int32_t v[9]);
int32_t oh_filter_temporal(int32_t c, int32_t p, int32_t n, int32_t mp, int32_t mn, int32_t threshold);

/* Histograms: the code values of n finished pictures counted plane by plane (the tests check every field bit for bit
 * against tests/levels_model.py).  The rules are those of oh_pics_compare: identical OhPicParams, win in luma samples with offsets that
 * are multiples of SubWidthC / SubHeightC, plane c's window is win shifted by oh_hshift / oh_vshift.  Reads finished halves on the engine
 * stream, waits for it and fills out on the host; every call starts from zero.  The GPU counts the bins; samples, sum, sum_sq, min and
 * max are derived from them on the host in 64-bit integers, so every field is exact and independent of the order of the workgroups.  A
 * stored sample above 2^bit_depth - 1, which no decoder and no service writes, counts in the top bin of its depth.  More than
 * OH_CONV_MAX_PICS pictures are split into several launches.  n == 0: OH_OK.
 * OH_E_ARG, out untouched: a null win, out or id array, a negative n, an unknown picture, pictures whose params differ, an empty window
 * or one whose offsets are not multiples of SubWidthC / SubHeightC.  No combination gives OH_E_UNSUPPORTED. */
enum { OH_HIST_BINS = 4096 };
typedef struct OhPlaneHist {
    uint64_t samples;              /* samples of the plane's window */
    uint64_t sum, sum_sq;          /* sum v, sum v^2 */
    uint32_t min, max;             /* of v; a plane the picture lacks: everything 0 */
    uint32_t hist[OH_HIST_BINS];   /* hist[v] = samples equal to v; bins >= 2^bit_depth are 0 */
} OhPlaneHist;
typedef struct OhHistogram { OhPlaneHist plane[3]; } OhHistogram;
int oh_pics_histogram(OhEngine *e, const int *pic_ids, int n, const OhWindow *win, OhHistogram *out);
/* host only: the n plane histograms pooled, N their samples (the sum of their bins), cum(v) the pooled count of the values <= v:
 * *value is the smallest v with cum(v) > 0 and cum(v) 10^6 >= ppm N, in 64-bit integers; ppm 0 gives the minimum, 10^6 the maximum.
 * OH_E_ARG: a null pointer, n < 1, ppm > 10^6, no samples. */
int oh_hist_percentile(const OhPlaneHist *h, int n, uint32_t ppm, uint32_t *value);
/* host only: *sad = sum over v of |a.hist[v] - b.hist[v]|, the scene-cut measure.  OH_E_ARG: a null pointer. */
int oh_hist_distance(const OhPlaneHist *a, const OhPlaneHist *b, uint64_t *sad);

/* Look-up tables: n finished pictures become n finished pictures of the same size and chroma format, every sample of a selected plane
 * c replaced by table[c][sample], over the whole coded planes (tests/levels_model.py).  The sources have identical
 * params among themselves, the destinations among themselves; both sides share width, height and chroma format, the bit depth may
 * differ.  A plane whose bit is clear is copied, which needs equal depths.  Bits of planes the format lacks are ignored, as are their
 * table pointers.  Reads finished halves, writes half 0 of each destination and marks it finished, like oh_pics_reformat; enqueued on the
 * engine stream, returns without waiting.  The tables are copied by the call (through a pinned buffer, onto the engine stream in front
 * of the launch): the host arrays may be freed on return.  n == 0: OH_OK (planes is checked all the same; n_entries and the tables are
 * not: there is no picture to take the depths from).  More than OH_CONV_MAX_PICS pictures are split into several launches.
 * OH_E_ARG, nothing written: a null e, lut or id array, a negative n; an unknown picture; params that differ as above; a destination
 * that is also a source, or listed twice; planes outside 0 .. 7; n_entries other than 2^(source bit depth); a null table of a selected
 * plane the format has; a table entry above 2^(destination bit depth) - 1; depths that differ while a plane the format has is not
 * selected.  No combination gives OH_E_UNSUPPORTED. */
typedef struct OhLut {
    int32_t planes;               /* bit c set: plane c goes through table[c]; clear: plane c is copied */
    int32_t n_entries;            /* must be 1 << (source bit depth) */
    const uint16_t *table[3];     /* HOST arrays of n_entries values, each 0 .. 2^(destination bit depth) - 1 */
} OhLut;
int oh_pics_lut(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhLut *lut);
/* host only: table builders, all in integers (division is the integer division of non-negative numbers, >> on a negative number an
 * arithmetic shift).  bs / bd: source / destination bit depth, each in {8, 9, 10, 12}; Ms / Md = 2^bs - 1 / 2^bd - 1; ks = 2^(bs - 8),
 * kd = 2^(bd - 8); out: 2^bs entries, v their index.  OH_E_ARG, out untouched: another depth, a null pointer, and what each one names.
 *   oh_lut_identity   s = bs - bd; s <= 0: v << -s; s > 0: min((v + 2^(s - 1)) >> s, Md) — oh_reformat_quantise with OH_RF_ROUND, f = 0
 *   oh_lut_range      to_full (non-zero: limited -> full, zero: full -> limited) of luma (chroma zero) or chroma (non-zero):
 *                       to full, luma       c = min(max(v, 16 ks), 235 ks) - 16 ks;  out = (c Md + (219 ks >> 1)) / (219 ks)
 *                       to full, chroma     d = min(max(v, 16 ks), 240 ks) - 128 ks;  m = (|d| Md + 112 ks) / (224 ks);
 *                                           out = min(max(2^(bd - 1) + sign(d) m, 0), Md)
 *                       to limited, luma    out = 16 kd + (v 219 kd + (Ms >> 1)) / Ms
 *                       to limited, chroma  d = v - 2^(bs - 1);  m = (|d| 224 kd + (Ms >> 1)) / Ms;
 *                                           out = min(max(128 kd + sign(d) m, 16 kd), 240 kd)
 *   oh_lut_linear     min(max(((v - pivot_in) gain_q16 + pivot_out 65536 + 32768) >> 16, 0), Md) in int64; the pivots are any int32;
 *                     gain -65536 with pivots 0 and Md inverts, 131072 doubles the contrast around the pivots
 *   oh_lut_stretch    auto-levels at one depth bd: lo = oh_hist_percentile(h, n, lo_ppm), hi = oh_hist_percentile(h, n, 10^6 - hi_ppm);
 *                     hi <= lo: the identity; else ((min(max(v, lo), hi) - lo) Md + ((hi - lo) >> 1)) / (hi - lo).
 *                     OH_E_ARG also: n < 1, lo_ppm + hi_ppm >= 10^6, no samples
 *   oh_lut_equalise   at one depth bd, the n histograms pooled: cum(v) the count of the values <= v, cmin = cum at the smallest value
 *                     present, N all samples; N == cmin: the identity; else 0 where cum(v) < cmin and
 *                     ((cum(v) - cmin) Md + ((N - cmin) >> 1)) / (N - cmin) elsewhere.  OH_E_ARG also: n < 1
 *   oh_lut_then       out[v] = second[first[v]] for v < n1: two tables in one pass.  OH_E_ARG: a null pointer, n1 or n2 below 1, an
 *                     entry of first that is >= n2 */
int oh_lut_identity(int bs, int bd, uint16_t *out);
int oh_lut_range(int bs, int bd, int to_full, int chroma, uint16_t *out);
int oh_lut_linear(int bs, int bd, int32_t gain_q16, int32_t pivot_in, int32_t pivot_out, uint16_t *out);
int oh_lut_stretch(const OhPlaneHist *h, int n, uint32_t lo_ppm, uint32_t hi_ppm, int bd, uint16_t *out);
int oh_lut_equalise(const OhPlaneHist *h, int n, int bd, uint16_t *out);
int oh_lut_then(const uint16_t *first, int n1, const uint16_t *second, int n2, uint16_t *out);

/* Film grain: n finished pictures become n finished pictures of identical params with synthesised grain added, as the film grain
 * characteristics SEI (ohevc_annexb.h: oh_sei_film_grain) asks of a decoder after its output process (the tests check
 * every coded plane bit for bit against tests/grain_model.py).  The profile of the message is SMPTE RDD 5's — model 0 (frequency
 * filtering), up to three model values (sigma, horizontal and vertical cut-off in sixteenths of the band, 2 .. 14), 8 x 8 blocks chosen
 * by their mean intensity, smoothing across block edges — but the synthesis is this project's own and NOT bit-exact with RDD 5, whose
 * Gaussian and seed tables it does not use: every sample is defined in integers below.
 * Definitions.  fmix(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16 in uint32.
 * H(a, b, c, d) = fmix(a ^ fmix(b ^ fmix(c ^ fmix(d ^ 0x9e3779b9)))).  gauss(h) = the sum of the four bytes of h, minus 510.
 * Pattern P[fh][fv], fh and fv in 2 .. 14, 32 x 32 int8: coefficients C[v][u] (int16, row v the vertical frequency) =
 * 8 gauss(H(1, 16 fh + fv, u, v)) where u < 2 fh, v < 2 fv and (u, v) != (0, 0), else 0; raw = HEVC's inverse 32 x 32 transform of C
 * at bit depth 8 (H.265 8.6.4.2: stage shifts 7 and 12, 16-bit clip between the stages); r = isqrt(sum raw^2 / 1024) (integer division,
 * floor square root); P = clip(-127, 127, floor((64 raw + r) / (2 r))).
 * A table per plane of 256 uint32_t, indexed by a block's 8-bit mean: entry = sigma | fh << 8 | fv << 12; sigma 0: no grain.
 * Block (bx, by) of plane c covers the samples x in 8 bx .. 8 bx + 7, y in 8 by .. 8 by + 7 that the coded plane has (n = 64, 32 or 16
 * of them: plane sizes are multiples of 4): a8 = ((sum of the samples + n / 2) / n) >> (bd - 8), entry = table[c][a8],
 * h = H(2, seed, c, 65536 by + bx), ox = ((h & 0xFFFF) 25) >> 16, oy = (((h >> 16) & 0x7FFF) 25) >> 15, negate = h >> 31.
 * Sample (x, y): p = +-P[fh][fv][oy + (y & 7)][ox + (x & 7)], g = (sigma p 2^(bd - 8) + 2^(4 + log2_scale)) >> (5 + log2_scale)
 * (arithmetic shift).  At x = 7 mod 8 with x + 1 < W and at x = 0 mod 8 with x > 0, g' = (g(x - 1) + 2 g(x) + g(x + 1) + 2) >> 2 from
 * the unsmoothed values of both blocks, elsewhere g' = g.  blending 0 (additive): out = clip(0, 2^bd - 1, s + g'); blending 1
 * (multiplicative, this project's definition): out = clip(0, 2^bd - 1, s + ((s g' + 2^(bd - 1)) >> bd)).  A plane whose bit in planes
 * is clear is copied.  seeds: one per picture — a caller passes the POC, so that a picture looks the same however often it is shown.
 * Bits of planes the format lacks are ignored, as are their table pointers.  Reads finished halves, writes half 0 of each destination
 * and marks it finished, like oh_pics_lut; enqueued on the engine stream, returns without waiting.  Tables and seeds are copied by the
 * call: the host arrays may be freed on return.  The 169 patterns (173 KB) are built on the first call of an engine and stay in device
 * memory.  n == 0: OH_OK (planes, blending and log2_scale are checked all the same).  More than OH_CONV_MAX_PICS pictures are split
 * into several launches.
 * OH_E_ARG, nothing written: a null e, g, seeds or id array, a negative n; an unknown picture; params that differ anywhere among the
 * 2n pictures; a destination that is also a source, or listed twice; planes outside 0 .. 7; blending outside 0 .. 1; log2_scale
 * outside 0 .. 15; a null table of a selected plane that the format has; an entry of such a table above 0xFFFF, or with a non-zero
 * sigma and a cut-off outside 2 .. 14.  No combination gives OH_E_UNSUPPORTED. */
enum { OH_GRAIN_ADDITIVE = 0, OH_GRAIN_MULTIPLICATIVE = 1 };
enum { OH_GRAIN_ENTRIES = 256 };
typedef struct OhGrain {
    int32_t planes;               /* bit c set: plane c gets grain by table[c]; clear: plane c is copied */
    int32_t blending;             /* OH_GRAIN_* */
    int32_t log2_scale;           /* 0 .. 15 */
    const uint32_t *table[3];     /* HOST tables of OH_GRAIN_ENTRIES entries */
} OhGrain;
int oh_pics_grain(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhGrain *g, const uint32_t *seeds);
/* host only: the pieces of the definition above, which the kernel shares (csrc/grain_common.h).
 *   oh_grain_hash      H(a, b, c, d);   oh_grain_gauss   gauss(h)
 *   oh_grain_pattern   pattern (fh, fv): coeffs and raw 1024 int16, pattern 1024 int8, row-major; any of the three may be null.
 *                      OH_E_ARG: a cut-off outside 2 .. 14
 *   oh_grain_uniform   all 256 entries of out = sigma | fh << 8 | fv << 12.  OH_E_ARG: a null out, sigma outside 0 .. 255, a cut-off
 *                      outside 2 .. 14
 *   oh_grain_from_sei  the tables of a message: per present component and interval, sigma = value 0, fh = value 1 (8 where the message
 *                      has one value), fv = value 2 (fh where it has fewer than three) over lower .. upper; intensities in no interval
 *                      and components without a model get entry 0.  out->planes from comp_model_present_flag, blending from
 *                      blending_mode_id, log2_scale from log2_scale_factor, table[c] = tables[c].  The separate colour description is
 *                      ignored: the grain is added to the decoded samples as they are.  OH_E_ARG: a null pointer, a message that is
 *                      absent (present 0) or cancelled.  OH_E_UNSUPPORTED: model_id other than 0, blending_mode_id above 1, more than
 *                      3 model values, a sigma outside 0 .. 255, a cut-off outside 2 .. 14, lower above upper, overlapping intervals
 *                      of one component; tables and out are untouched then
 *   oh_grain_block     ox, oy, negate of block (bx, by), each 0 .. 65535, of plane c (0 .. 2).  OH_E_ARG: outside those, a null pointer
 *   oh_grain_mean      a8 of a block of n (64, 32 or 16) samples of bd bits (8, 9, 10, 12) that sum to sum; -1: other n or bd
 *   oh_grain_value     g of a pattern value p (-127 .. 127, signed by negate), sigma 0 .. 255, log2_scale 0 .. 15 at bd bits (8, 9, 10,
 *                      12): |g| <= 16193, far inside OH_GRAIN_MAX.  0 outside these domains
 *   oh_grain_smooth    g' of a sample at a block edge: (left + 2 g + right + 2) >> 2.  0 unless all three lie in +-OH_GRAIN_MAX
 *   oh_grain_blend     out of a sample s (0 .. 2^bd - 1) and its g' (+-OH_GRAIN_MAX), blending 0 or 1.  0 outside these domains */
enum { OH_GRAIN_MAX = 1 << 18 };
uint32_t oh_grain_hash(uint32_t a, uint32_t b, uint32_t c, uint32_t d);
int32_t oh_grain_gauss(uint32_t h);
int oh_grain_pattern(int fh, int fv, int16_t *coeffs, int16_t *raw, int8_t *pattern);
int oh_grain_uniform(int sigma, int fh, int fv, uint32_t *out);
struct OhFilmGrainSei;
int oh_grain_from_sei(const struct OhFilmGrainSei *sei, uint32_t tables[3][256], OhGrain *out);
int oh_grain_block(uint32_t seed, int c, int bx, int by, int *ox, int *oy, int *negate);
int32_t oh_grain_mean(uint32_t sum, int n, int bit_depth);
int32_t oh_grain_value(int32_t sigma, int32_t p, int bit_depth, int log2_scale);
int32_t oh_grain_smooth(int32_t left, int32_t g, int32_t right);
int32_t oh_grain_blend(int32_t s, int32_t g, int bit_depth, int blending);

/* Colour remapping: n finished 4:4:4 pictures become n finished 4:4:4 pictures of the same size, every output sample made from all
 * three components of the source sample, as the colour remapping information SEI (ohevc_annexb.h: oh_sei_colour_remap) prescribes: a
 * table per component, a 3 x 3 matrix, a second table per component (the tests check every coded plane bit for bit
 * against tests/remap_model.py).  Everything is in integers.  bi / bo: the input / output bit depth, each 8, 9, 10 or 12;
 * Mi = 2^bi - 1, Mo = 2^bo - 1.  Sample (s0, s1, s2): p_i = pre[i][s_i]; m_c = clip(0, Mo, (sum_i coeff[c][i] p_i + r) >> d) with
 * d = log2_denom, r = 2^(d - 1) for d > 0 and 0 for d = 0, the shift arithmetic; out_c = post[c][m_c].  A source sample above Mi, which
 * no decoder and no service writes, is looked up by its low bits.  Sources are of in_bit_depth, destinations of out_bit_depth, over the
 * whole coded planes.  Reads finished halves, writes half 0 of each destination and marks it finished, like oh_pics_lut; enqueued on the
 * engine stream, returns without waiting.  The tables are copied by the call: the host arrays may be freed on return.  n == 0: OH_OK
 * after the checks that need no picture (the struct's).  More than OH_CONV_MAX_PICS pictures are split into several launches.
 * OH_E_ARG, nothing written: a null e, r or id array, a negative n; an unknown picture; params that differ among the sources or among
 * the destinations; a destination that is also a source, or listed twice; sizes that differ; a picture depth other than the struct's; a
 * struct depth outside 8, 9, 10, 12; a null table; a table entry above Mo; a coefficient outside -32768 .. 32767; log2_denom outside
 * 0 .. 15.  OH_E_UNSUPPORTED: a chroma format other than 4:4:4 on either side (oh_pics_reformat first, or oh_remap_luts with oh_pics_lut
 * where the matrix is diagonal). */
typedef struct OhRemap {
    int32_t in_bit_depth, out_bit_depth;
    const uint16_t *pre[3];       /* HOST, 2^in entries, values 0 .. Mo  */
    int32_t coeff[3][3], log2_denom;
    const uint16_t *post[3];      /* HOST, 2^out entries, values 0 .. Mo */
} OhRemap;
int oh_pics_colour_remap(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhRemap *r);
/* host only: the pieces of the definition above, which the kernel shares (csrc/remap_common.h).
 *   oh_remap_curve     the piecewise-linear table of 2^bi_ entries from bi_ to bo_ bits (each 8, 9, 10 or 12, passed independently: a
 *                      post curve is bo -> bo) through n pivots (coded[k], target[k]).  n = 0: the points (0, 0), (Mi_, Mo_).  Otherwise
 *                      the n given points (n <= 33), a point (0, 0) in front where coded[0] > 0 and a point (Mi_, Mo_) behind where the
 *                      last coded value is below Mi_.  For v in x_k .. x_k+1, dx = x_k+1 - x_k, t = v - x_k:
 *                      out[v] = (y_k (dx - t) + y_k+1 t + (dx >> 1)) / dx.  Targets need not be monotonic.  OH_E_ARG, out untouched: a
 *                      null pointer (coded and target may be null where n is 0), another depth, n outside 0 .. 33, coded values not
 *                      strictly increasing, a coded value above Mi_, a target above Mo_
 *   oh_remap_sample    out[3] of the sample s[3]; 1, or 0 for a null pointer or an OhRemap that oh_pics_colour_remap would refuse
 *   oh_remap_from_sei  the six curves of a message in tables (0 .. 2 pre, 3 .. 5 post; num_val_minus1 of 0 is a curve without pivots),
 *                      its matrix (absent: the identity with log2_denom 0), out pointing into tables.  The signal info describes the
 *                      result and changes no sample: it is passed over.  OH_E_ARG: a null pointer, a message that is absent (present 0)
 *                      or cancelled, what oh_remap_curve refuses.  OH_E_UNSUPPORTED: a depth outside 8, 9, 10, 12.  tables and out are
 *                      untouched then
 *   oh_remap_luts      where every off-diagonal coefficient is 0 the remap is a function of each plane alone:
 *                      out[c][v] = post[c][clip(0, Mo, (coeff[c][c] pre[c][v] + r) >> d)] for v < 2^bi, tables for oh_pics_lut, which
 *                      works at any chroma format.  OH_E_ARG: a null pointer or an OhRemap that oh_pics_colour_remap would refuse;
 *                      OH_E_UNSUPPORTED: any other matrix; out is untouched then */
int oh_remap_curve(int in_bit_depth, int out_bit_depth, int n, const uint16_t *coded, const uint16_t *target, uint16_t *out);
int oh_remap_sample(const OhRemap *r, const uint16_t s[3], uint16_t out[3]);
struct OhColourRemapSei;
int oh_remap_from_sei(const struct OhColourRemapSei *sei, uint16_t tables[6][4096], OhRemap *out);
int oh_remap_luts(const OhRemap *r, uint16_t out[3][4096]);

/* Frame packing: a finished picture that holds the two views of a stereo pair, as the frame packing arrangement SEI (ohevc_annexb.h:
 * oh_sei_frame_packing) describes it, becomes two finished pictures, one per view, and two views become a packed picture (DESIGN.md
 * §3s; the tests check every coded plane bit for bit against tests/packing_model.py).  Everything is in integers, per plane and in the
 * plane's own coordinates.  In a plane of the packed picture, view v (constituent frame v) occupies the rectangle R_v: the left half
 * (OH_PACK_SIDE_BY_SIDE) or the top half (OH_PACK_TOP_BOTTOM) for v = 0, the other half for v = 1.  C_v[y][x] is R_v read with the
 * flip undone: with flip[v], columns mirrored inside R_v (side by side) or rows mirrored inside R_v (top-bottom).  The size of the
 * views picks the mode.  With packed pictures of W x H luma samples (shifts hs, vs of the chroma planes):
 *   half size   (W / 2) x H side by side, W x (H / 2) top-bottom: D_v = C_v, with or without quincunx.  oh_pics_pack with half-size
 *               views is the exact inverse: it places the views and re-applies the flips.
 *   full size   W x H, no quincunx: a 1-D up-sampling by two along the packed axis (x side by side, y top-bottom) on the phase the grid
 *               position gives; the other axis is copied.  Taps c[16][8] for luma and c[16][4] for chroma: the 16-phase SHVC tables.
 *               With g = grid_x[v] (side by side) or grid_y[v] (top-bottom), output index Z on the packed axis has the position p, in
 *               1/16 of the spacing of the stored samples: p = 8 Z - g where the plane is not sub-sampled on the packed axis;
 *               p = (16 Z - g + 1) >> 1 on a sub-sampled horizontal axis (co-sited chroma); p = (16 Z - g - 3) >> 1 on a sub-sampled
 *               vertical axis (chroma midway between luma rows, chroma_sample_loc_type 0); >> floors.  i = p >> 4, phase = p & 15,
 *               S = sum_k c[phase][k] C_v[clamp(i + k - 3, 0, N - 1)] with 8 taps (k - 1 with 4 taps), N the view's own stored samples
 *               on that axis — a tap never reaches across the seam into the other view —, D = clip((S + 32) >> 6, 0, 2^bd - 1).
 *               The other grid component (grid_y side by side, grid_x top-bottom) is carried and not applied.
 *   quincunx    this project's reading of the lattice: side by side C_v[y][x] is the full-resolution sample (2 x + ((y + v) & 1), y),
 *               top-bottom (x, 2 y + ((x + v) & 1)); frame 0 holds (0, 0).  Full-size views: lattice samples are copied, every other
 *               sample is (L + R + U + D + 2) >> 2 of its four lattice neighbours, a neighbour outside the plane replaced by the
 *               opposite one.  oh_pics_pack with quincunx takes full-size views and point-samples the lattice: it does not pre-filter.
 * A view's picture has the packed pictures' params but for its size, whose sides are rounded up to the minimum coding block
 * (oh_packing_view_size): the view is the top-left window of it, and the rest of the coded planes replicates the window's last column
 * and last row, as in oh_pics_orient.  Where the half size rounds up to the full size (a packed side of one minimum coding block), the
 * full size is meant.  oh_pics_unpack: view0_ids or view1_ids may be null, that view is then not made.  Both calls read finished
 * halves, write half 0 of each destination and mark it finished, like oh_pics_orient; enqueued on the engine stream, they return
 * without waiting.  n == 0: OH_OK after the checks of the descriptor.  More than OH_PK_MAX_PICS = 32 packed pictures are split into
 * several launches.
 * OH_E_ARG, nothing written: a null e, pk or packed id array, both view arrays null (oh_pics_pack: either), a negative n; an
 * arrangement other than 3 or 4, quincunx or a flip outside 0 / 1, a grid position outside 0 .. 15; an unknown picture; params that
 * differ among the packed pictures or among the views; a picture that is both source and destination, or a destination listed twice;
 * a packed width that is no multiple of 2 << hs (side by side) or height that is no multiple of 2 << vs (top-bottom): each half is a
 * whole number of chroma samples; views that are of neither size; oh_pics_pack with quincunx and half-size views.
 * OH_E_UNSUPPORTED, nothing written: views of another bit depth or chroma format than the packed pictures (oh_pics_reformat first);
 * oh_pics_pack without quincunx and full-size views: the anti-aliased 2 : 1 is oh_pics_resize's, then pack the halves. */
enum { OH_PACK_SIDE_BY_SIDE = 3, OH_PACK_TOP_BOTTOM = 4 };     /* frame_packing_arrangement_type */
enum { OH_PK_MAX_PICS = 32 };
typedef struct OhPacking {
    int32_t arrangement;              /* OH_PACK_SIDE_BY_SIDE or OH_PACK_TOP_BOTTOM */
    int32_t quincunx;                 /* 0 / 1 */
    int32_t flip[2];                  /* view v is stored mirrored: horizontally side by side, vertically top-bottom */
    int32_t grid_x[2], grid_y[2];     /* 0 .. 15: the position of view v's top-left sample, in 1/16 of the stored sample spacing */
    int32_t content_interpretation;   /* carried: 1 frame 0 is the left view, 2 frame 1 is; changes no sample */
} OhPacking;
int oh_pics_unpack(OhEngine *e, const int *src_ids, const int *view0_ids, const int *view1_ids, int n, const OhPacking *pk);
int oh_pics_pack(OhEngine *e, const int *view0_ids, const int *view1_ids, const int *dst_ids, int n, const OhPacking *pk);
/* host only: the pieces of the definition above, which the kernels share (csrc/packing_common.h).
 *   oh_packing_from_sei     the descriptor of a message: arrangement types 3 and 4; flip[v] is 1 for the constituent frame that is stored
 *                           mirrored (spatial_flipping_flag, and frame0_flipped_flag names frame v).  OH_E_UNSUPPORTED: type 5 (temporal
 *                           interleaving: nothing to unpack, current_frame_is_frame0_flag says which view a picture is), types 0 .. 2
 *                           and above 5, which HEVC does not define, field_views_flag; oh_packing_unsupported says which in words
 *                           ("" for a message that is supported).  OH_E_ARG: a null pointer, a message that is absent or cancelled,
 *                           a grid position outside 0 .. 15.  out is untouched then
 *   oh_packing_view_size    the params of a view of half (full 0) or full (full 1) size of packed pictures of params `packed`.
 *                           OH_E_ARG: a null pointer, full outside 0 / 1, what the calls refuse of the descriptor and the packed size
 *   oh_packing_sample       *out: sample (x, y) of coded plane `plane` of view `view` of that size, from `samples`, the packed picture's
 *                           plane `plane` (uint8_t at 8 bit, else uint16_t; `stride` samples between rows).  OH_E_ARG as above, or a
 *                           position outside the view's coded plane
 *   oh_packing_pack_sample  *out: sample (x, y) of plane `plane` of the packed picture from the same plane of the two views (half size,
 *                           with quincunx full size; `stride` samples between the rows of either)
 *   oh_packing_views        *left, *right: the constituent frame that is the left / the right view: content_interpretation 1, frame 0
 *                           is the left view; 2, frame 1 is.  Returns 1, or 0 (nothing written) for a null pointer and where the
 *                           interpretation is unspecified (0) or reserved */
struct OhFramePackingSei;
int oh_packing_from_sei(const struct OhFramePackingSei *sei, OhPacking *out);
const char *oh_packing_unsupported(const struct OhFramePackingSei *sei);
int oh_packing_view_size(const OhPacking *pk, const OhPicParams *packed, int full, OhPicParams *view);
int oh_packing_sample(const OhPacking *pk, const OhPicParams *packed, int full, int view, int plane, int x, int y, const void *samples,
                      int stride, int32_t *out);
int oh_packing_pack_sample(const OhPacking *pk, const OhPicParams *packed, int plane, int x, int y, const void *view0, const void *view1,
                           int stride, int32_t *out);
int oh_packing_views(const OhPacking *pk, int *left, int *right);

/* Motion: a block-matching search between two finished pictures and the motion-compensated prediction that such a field describes, in
 * HEVC's quarter-sample units with HEVC's interpolation filters, so that a vector means what it means to an HEVC decoder (DESIGN.md
 * §3o; the tests check every field and every plane bit for bit against tests/motion_model.py, which is held against the oracle's
 * uni-prediction at every fraction).
 * Definitions.  W x H the coded luma plane, M = 2^bit_depth - 1.  Rows and columns of the reference clamp to the plane (HEVC's
 * padding), so every vector is defined.  Block (bx, by) of size B is the luma rectangle at (bx B, by B) of B x B samples cut at the
 * plane's edge (sizes are multiples of 8, so B = 16 leaves blocks 8 wide or high).  P(mv) is the luma prediction of that rectangle
 * from ref with the vector mv, the uni-predicted samples of H.265 8.5.3.3.3: xInt = x + (mvx >> 2), xFrac = mvx & 3, likewise y; the
 * 8-tap filters {-1,4,-10,58,17,-5,1,0}, {-1,4,-11,40,40,-11,4,-1}, {0,1,-5,17,58,-10,4,-1} over the columns xInt - 3 .. xInt + 4;
 * the first stage shifted right by bit_depth - 8; with both fractions non-zero a second stage over eight rows of first-stage values,
 * shifted right by 6; without any fraction the sample << (14 - bit_depth); that 14-bit value v becomes
 * min(max((v + 2^(13 - bit_depth)) >> (14 - bit_depth), 0), M).  SAD(mv) = sum |cur - P(mv)| over the rectangle.  With the block's
 * centre c = (cx, cy) in integer samples and d(mv) = |mvx - 4 cx| + |mvy - 4 cy|: cost(mv) = SAD(mv) + ((lambda d(mv)) >> 2).
 * Candidates are ordered by the key (cost, d, mvy, mvx), ascending and lexicographic: a total order, so the winner does not depend on
 * the order of evaluation.
 *
 * oh_pics_motion: per pair (cur_ids[i], ref_ids[i]) and block, stage 0 tries the (2 range_x + 1)(2 range_y + 1) integer vectors
 * 4 (c + (i, j)), |i| <= range_x, |j| <= range_y, and takes the smallest key; with subpel >= 1 stage 1 tries the stage-0 winner +
 * {-2, 0, 2}^2; with subpel == 2 stage 2 tries the stage-1 winner + {-1, 0, 1}^2.  out[(i bh + by) bw + bx] (bw, bh:
 * oh_motion_blocks) receives the winner, its SAD and SAD(4 c).  Only luma is searched.  All pictures have identical params; a picture
 * may appear in many pairs and as both members of one.  Nothing is written to pictures.  centres: per pair and block (cx, cy), int16,
 * in the order of out; copied by the call through a pinned buffer onto the engine stream.  Reads finished halves on the engine stream,
 * waits for it and fills out on the host.  More than OH_CONV_MAX_PICS pairs are split into several launches.  n == 0: OH_OK (ms is
 * checked all the same, but for the centres, of which there are none).
 * OH_E_ARG, out untouched: a null e, ms, out or id array, a negative n; an unknown picture; params that differ; block other than 8 or
 * 16; a range outside 0 .. OH_MOTION_MAX_RANGE; subpel outside 0 .. 2; lambda outside 0 .. OH_MOTION_MAX_LAMBDA; a centre component
 * beyond +-OH_MOTION_MAX_CENTRE.  No combination gives OH_E_UNSUPPORTED.
 *
 * oh_pics_motion_compensate: n finished ref pictures become n finished dst pictures of identical params.  field: n bw bh vectors in
 * the order of out above, of which only x and y are read; any int16 value is legal.  Luma of block (bx, by) of dst is P(its vector).
 * Each chroma plane of the block is the rectangle divided by SubWidthC / SubHeightC, predicted by H.265 8.5.3.3.3 chroma (hs / vs =
 * oh_hshift / oh_vshift): xIntC = xC + (mvx >> (2 + hs)), the eighth-sample fraction (mvx & ((4 << hs) - 1)) << (1 - hs), likewise y
 * with vs; the 4-tap filters {-2,58,10,-2}, {-4,54,16,-2}, {-6,46,28,-4}, {-4,36,36,-4} and their mirror images over the columns
 * xIntC - 1 .. xIntC + 2, the stages, shifts and rounding of luma.  A 4:0:0 picture has no chroma.  Writes half 0 of each destination
 * and marks it finished; enqueued on the engine stream, returns without waiting, like oh_pics_filter.  The field is copied by the
 * call.  A zero field gives a copy of ref.  n == 0: OH_OK (block is checked all the same).
 * OH_E_ARG, nothing written: a null e, field or id array, a negative n; an unknown picture; params that differ; a destination that is
 * also a source, or listed twice; block other than 8 or 16. */
enum { OH_MOTION_MAX_RANGE = 32, OH_MOTION_MAX_CENTRE = 4096, OH_MOTION_MAX_LAMBDA = 4096 };
typedef struct OhMotionVector { int16_t x, y;        /* quarter luma samples, HEVC's mvLX */
                                uint32_t sad;        /* SAD of the winner */
                                uint32_t sad_centre; /* SAD at the block's search centre (integer vector) */ } OhMotionVector;
typedef struct OhMotionSearch {
    int32_t block;            /* 8 or 16 */
    int32_t range_x, range_y; /* 0 .. OH_MOTION_MAX_RANGE, integer samples either side of the centre */
    int32_t subpel;           /* 0 integer, 1 half, 2 quarter */
    int32_t lambda;           /* 0 .. OH_MOTION_MAX_LAMBDA */
    const int16_t *centres;   /* NULL (all zero) or HOST array: per pair, per block, (cx, cy) in integer samples, |c| <= OH_MOTION_MAX_CENTRE */
} OhMotionSearch;
int oh_motion_blocks(int width, int height, int block, int *bw, int *bh);       /* host only: ceil(W / block), ceil(H / block) */
int oh_pics_motion(OhEngine *e, const int *cur_ids, const int *ref_ids, int n, const OhMotionSearch *ms, OhMotionVector *out);
int oh_pics_motion_compensate(OhEngine *e, const int *ref_ids, const int *dst_ids, int n, int block, const OhMotionVector *field);
/* host only, coarse to fine: a field searched with blocks of block_c on pictures reduced by the integer factor s in {1, 2, 4, 8}
 * (bwc x bhc blocks) becomes the search centres of a grid of bw x bh blocks of block_f on the full pictures.  Fine block (bx, by)
 * takes the coarse block (min(bx block_f / (s block_c), bwc - 1), min(by block_f / (s block_c), bhc - 1)); its centre is
 * (s mv + 2) >> 2 per component (an arithmetic shift), clamped to +-OH_MOTION_MAX_CENTRE; centres: 2 bw bh int16, (cx, cy) per block.
 * OH_E_ARG, centres untouched: a null pointer, a size below 1, another s, a block size other than 8 or 16. */
int oh_motion_scale(const OhMotionVector *coarse, int bwc, int bhc, int block_c, int s, int bw, int bh, int block_f, int16_t *centres);
/* host only: the formulas above as the kernels evaluate them (csrc/motion_common.h).  oh_motion_qpel: win the 8 x 8 reference
 * samples of rows yInt - 3 .. yInt + 4 and columns xInt - 3 .. xInt + 4, row by row; fx, fy in 0 .. 3.  oh_motion_epel: win the 4 x 4
 * samples of rows yIntC - 1 .. yIntC + 2 and columns xIntC - 1 .. xIntC + 2; fx, fy in 0 .. 7.  Both return the predicted sample, or
 * -1 for a null window, a fraction outside its range or a bit depth other than 8, 9, 10, 12.  oh_motion_cost: sad + ((lambda d) >> 2)
 * of the vector (mvx, mvy) around the centre (cx, cy), in 64 bits so that it is defined for every argument. */
int32_t oh_motion_qpel(const uint16_t win[64], int fx, int fy, int bit_depth);
int32_t oh_motion_epel(const uint16_t win[16], int fx, int fy, int bit_depth);
uint64_t oh_motion_cost(uint32_t sad, int mvx, int mvy, int cx, int cy, int lambda);

/* SHVC inter-layer reference picture: resample the finished base-layer picture src_pic into
 * the enhancement-layer picture dst_pic, bit-exact with the reference's whole-picture slot
 * HEVCDSPContext.upsample_base_layer_frame (hevcdsp_template.c:2164-2438, call site hevc.c:3241).
 * 8-bit 4:2:0 only, like that routine (OH_E_UNSUPPORTED otherwise).  u: oh_upsample_setup().
 * The reference's default build never calls that slot (ACTIVE_PU_UPSAMPLING hevc.h:117): what it decodes is the CTB path of
 * oh_pic_upsample_blocks below, which differs with offsets, phase alignment and x1.5 beyond 2048 EL columns / rows. */
int oh_pic_upsample(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u);
/* The same resampling for a LIST of CTBs of the enhancement-layer picture (raster addresses for CTBs of 1 << log2_ctb_size luma
 * samples; the rest of dst_pic is left as it is): the granularity of the reference's default build, which up-samples a CTB when
 * a prediction unit first reads the inter-layer reference there (ACTIVE_PU_UPSAMPLING hevc.h:117, ff_upsample_block
 * hevc_filter.c:1370-1426, is_upsampled[]).  A decoder collects the CTBs its picture's inter-layer PUs touch and issues one call
 * before the picture's work list.  Same samples as the reference's CTB path wherever that path and its whole-picture slot agree:
 * no scaled reference layer offsets and no phase alignment (tests/test_upsample_vs_ref.py); offsets are refused
 * (OH_E_UNSUPPORTED — use oh_pic_upsample).  The motion-field half of that path (ff_upscale_mv_block, hevc_filter.c:1311-1368)
 * feeds merge / AMVP derivation (hevc_mvs.c), host work by SURVEY §8, and stays with the host decoder.
 * For the reference's own CTB arithmetic everywhere it is defined (offsets, phase alignment, x1.5 at any size): oh_pic_upsample_blocks. */
int oh_pic_upsample_ctbs(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u, int log2_ctb_size, const uint32_t *ctb_addrs, int n);
/* The reference's CTB path itself: per listed EL CTB what its block driver computes (upsample_block_luma / upsample_block_mc,
 * hevc_filter.c:1175-1309) — its base-layer window estimates and margins, one emulated edge per call (emulated_edge_up_h / _v,
 * videodsp_template.c:103-160) and the slot variant u->idx picks (upsample_filter_block_*, hevcdsp_template.c:1834-2162: x2 fixed
 * phases, x1.5 exact thirds, the 16.16 generic one, a copy at x1).  ctb_addrs == NULL: every CTB (n ignored); CTBs not listed keep
 * their samples, and so do chroma rows outside the scaled reference layer window (the chroma v slots store at the clipped row).
 * Where the reference's CTB path reads samples no call of its own wrote (see oh_upsample_blocks_defined) the call returns
 * OH_E_UNSUPPORTED and names the CTB and the reason; it never computes something else.  el_conf_win: the enhancement layer's
 * conformance window, by which the driver positions (hevc_filter.c:1196-1197, 1257-1258); only an empty one (or NULL) for now.
 * 8-bit 4:2:0 only. */
int oh_pic_upsample_blocks(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u, int log2_ctb_size,
                           const OhWindow *el_conf_win, const uint32_t *ctb_addrs, int n);
/* Host only (no device needed): 1 when every CTB of the picture pair, up-sampled by the reference's CTB path with an empty EL
 * conformance window, reads only samples that its own call wrote or the base layer holds; 0 otherwise, with *first_bad_ctb the
 * first such CTB (raster address; -1 when the scale itself is out of range).  It is 0 where a CTB's vertical slot reads an
 * intermediate row the short window estimate (hevc_filter.c:1260 "FIXME") did not filter — scratch of an earlier call, so the
 * result depends on call order —, reads base-layer samples beyond an edge its call did not emulate (one edge per call:
 * videodsp_template.c:110-116, 141-151, e.g. an EL of a single CTB row or column) or base-layer rows the picture does not have
 * (the chroma height of hevc_filter.c:1252 at vertical ratios above 2), overwrites base-layer samples with its left edge
 * emulation, or stores chroma rows of another CTB.  The edge replications themselves are deterministic and are reproduced.
 * OH_E_ARG for a bad geometry. */
int oh_upsample_blocks_defined(const OhUpsample *u, int w_bl, int h_bl, int w_el, int h_el, int log2_ctb_size, int *first_bad_ctb);

/* work lists.  OhFrame.cur_pic / ref_pics[] hold engine picture ids.
 * upload copies every array to HBM (after it returns the host arrays may be reused);
 * execute enqueues passes 1-5 on the engine stream and may be called repeatedly on the same
 * device frame (the coefficient pool is never modified). */
int oh_frame_upload(OhEngine *e, const OhFrame *f, OhDevFrame **out);
/* n work lists at once (what a batch of independent pictures that will run as one oh_frames_execute should use): every chunk of up to
 * 32 lists shares ONE device arena, is copied with a few large requests and prepared by ONE set of launches.  All or nothing: on
 * error no list stays uploaded.  The lists are still executed, released and freed one by one and in any order, but the device
 * memory of the lists of one chunk is returned TOGETHER, when the last of them is released or freed: a caller that keeps one list
 * of a call for long keeps the memory of the whole chunk. */
int oh_frames_upload(OhEngine *e, const OhFrame *const *fs, int n, OhDevFrame **out);
int oh_frame_execute(OhEngine *e, OhDevFrame *df);
/* n mutually independent pictures (none is a reference of another one; same OhPicParams): every pass
 * is ONE launch over all of them, which is how pictures of independent sequences / GOPs (the reference's
 * frame threads, pthread_frame.c) fill the GPU while each picture's own dependency chain is short of it */
int oh_frames_execute(OhEngine *e, OhDevFrame *const *dfs, int n);      /* n == 0: nothing to do, OH_OK */
int oh_frame_free(OhEngine *e, OhDevFrame *df);          /* waits for the engine stream, then frees */
/* same without the wait: legal right after the last oh_frame(s)_execute of df was ENQUEUED — the device memory is recycled in
 * stream order (a decoder that uploads, executes and forgets one work list per picture never blocks on the GPU) */
int oh_frame_release(OhEngine *e, OhDevFrame *df);
/* the boundary-strength grids of an uploaded work list as the deblock pass will read them: the ones handed over, or — with
 * OhFrame.bs_in — the ones the engine derived from the motion field at upload (hevc_filter.c:584-941).
 * bytes: size of each destination, at most oh_bs_size() is copied */
int oh_frame_download_bs(OhEngine *e, OhDevFrame *df, uint8_t *vbs, uint8_t *hbs, size_t bytes);
int oh_frame_submit(OhEngine *e, const OhFrame *f);     /* upload + execute + release in stream order: nothing of the list stays behind */
/* what the engine holds for work lists: out[0] device arenas alive (pooled or holding the lists of one upload call), [1] their bytes, [2] of them free in the pool,
 * [3] pinned staging buffers, [4] their bytes, [5] work lists waiting for a deferred free.  A decoder that submits and forgets one list
 * per picture sees all of them level off after a few pictures, however long the stream. */
int oh_engine_memory(OhEngine *e, uint64_t out[6]);

/* per-pass device time of the executes since the last reset, measured with HIP events on the
 * engine stream (enable = 1 costs two event records per pass; enable = 2 additionally brackets every
 * launch of the intra pass, see oh_engine_intra_launch_times).  ms[] and launches[] hold OH_N_PASSES
 * entries: accumulated milliseconds and number of timed executes. */
int oh_engine_profile(OhEngine *e, int enable);
int oh_engine_pass_times(OhEngine *e, double *ms, uint64_t *executes, int reset);
/* the intra pass is one launch per CTU-wavefront level: summed per-launch device time and launch
 * count (events bracket every launch in profile mode); read after oh_engine_pass_times() */
int oh_engine_intra_launch_times(OhEngine *e, double *ms, uint64_t *launches, int reset);

/* where the HOST time of the hand-over path went since the last reset: accumulated wall milliseconds and calls per OH_HT_* slot
 * (nested: OH_HT_UPLOAD contains the OH_HT_UPLOAD_* parts, OH_HT_EXECUTE contains OH_HT_EXECUTE_WAIT_PREP) */
enum OhHostTime { OH_HT_UPLOAD = 0, OH_HT_UPLOAD_COUNT, OH_HT_UPLOAD_ARENA, OH_HT_UPLOAD_STAGE_WAIT, OH_HT_UPLOAD_MEMCPY, OH_HT_UPLOAD_ENQUEUE,
                  OH_HT_EXECUTE, OH_HT_EXECUTE_WAIT_PREP, OH_HT_RELEASE, OH_N_HOST_TIMES };
int oh_engine_host_times(OhEngine *e, double *ms, uint64_t *calls, int n, int reset);
uint64_t oh_engine_upload_bytes(OhEngine *e, int reset);      /* bytes of work lists copied host -> device since the last reset */

/* the stream everything is enqueued on (hipStream_t as void*), for callers that need to order
 * their own work (RCCL broadcasts of reference pictures) against the engine */
void *oh_engine_stream(OhEngine *e);
/* device address / geometry of a picture's FINAL planes (valid after the frame that writes it was
 * executed), for zero-copy exchange between GPUs; stride in samples */
int oh_pic_device_planes(OhEngine *e, int pic_id, void *planes[3], int32_t stride[3], int32_t width[3], int32_t height[3]);

/* diagnostics only: in-kernel cycle stamps of a -DOH_STAMPS build (tools/intra_stamps.py) */
int oh_debug_read(OhEngine *e, uint64_t *out, size_t n_u64);

#ifdef __cplusplus
}
#endif
#endif
