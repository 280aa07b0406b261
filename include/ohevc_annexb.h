/*
 * ohevc_annexb.h — the byte-stream side of the path (C ABI, host only, part of libohevc_host.so): what sits
 * between a raw .bit / .bin file and the host decoder that fills the work lists, and what the picture-hash check needs from the stream.
 *
 *   access-unit splitter     libavcodec/hevc_parser.c:40-87   hevc_find_frame_end (the parser the reference's harness reads raw files through)
 *   NAL unit scan of an AU   libavcodec/hevc.c:3854-3893      decode_nal_units' start-code search + hls_nal_unit's header (hevc.c:3672-3697)
 *   NAL unescape             libavcodec/hevc.c:3724-3829      ff_hevc_extract_rbsp (emulation-prevention bytes out, their positions kept)
 *   picture-hash SEI         libavcodec/hevc_sei.c:28-50,134-181   decode_nal_sei_message / decode_nal_sei_decoded_picture_hash
 *
 * Entropy decoding (CABAC, hevc_cabac.c) is NOT here: it stays on the host decoder (out of scope).
 */
#ifndef OHEVC_ANNEXB_H
#define OHEVC_ANNEXB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OH_AU_END_NOT_FOUND (-100)          /* parser.h END_NOT_FOUND */

/* streaming state of the splitter (hevc_parser.c's ParseContext.state64 / frame_start_found) */
typedef struct OhAuScanner { uint64_t state64; int32_t frame_start_found; int32_t reserved; } OhAuScanner;
void oh_au_scanner_init(OhAuScanner *sc);
/* Feed the next `size` bytes.  Returns the offset in `buf` of the first byte of the NEXT access unit — the first zero of the
 * three-byte start code that opens it; negative down to -5 when that start code began in the bytes of an earlier call — or
 * OH_AU_END_NOT_FOUND.  A new access unit begins at the first VPS / SPS / PPS / AUD / prefix-SEI / reserved 41-44, 48-55 NAL unit of
 * layer 0 that follows a picture's first slice segment, or at the next slice segment with first_slice_segment_in_pic_flag = 1. */
long oh_au_find_frame_end(OhAuScanner *sc, const uint8_t *buf, size_t size);
/* Whole buffer: offsets[0] = 0, offsets[k] = start of access unit k, offsets[n] = size; returns n (needs cap >= n + 1), or -(n + 1)
 * when cap is too small (nothing written past cap). */
long oh_annexb_split(const uint8_t *data, size_t size, size_t *offsets, size_t cap);

typedef struct OhNal {
    size_t  offset;                         /* of the first header byte (behind the start code) in the buffer scanned */
    size_t  size;                           /* escaped bytes up to the next start code / trailing zeros (header included) */
    int32_t type, layer_id, temporal_id;    /* nal_unit_type, nuh_layer_id, nuh_temporal_id_plus1 - 1 */
    int32_t first_slice_segment_in_pic;     /* VCL NAL units: the flag; others 0 */
} OhNal;
/* NAL units of one access unit (or any Annex-B buffer).  Returns their number (at most cap written), or -1 when bytes other than
 * zeros precede a start code ("No start code is found", hevc.c:3876). */
long oh_annexb_nal_units(const uint8_t *buf, size_t size, OhNal *out, size_t cap);

/* RBSP of one NAL unit: src[0 .. length) starts at the NAL header; dst needs `length` bytes.  Emulation-prevention bytes (00 00 03)
 * are dropped and the position in dst of the byte before each one — as ff_hevc_extract_rbsp keeps them for the entry-point
 * arithmetic of hls_slice_data_wpp (hevc.c:2829-2842) — goes to skipped_pos (up to cap; *n_skipped counts all).  Stops at the next
 * start code (00 00 00 / 00 00 01 / 00 00 02).  Returns the bytes of src consumed. */
long oh_nal_unescape(const uint8_t *src, size_t length, uint8_t *dst, size_t *dst_size, int32_t *skipped_pos, size_t cap, int32_t *n_skipped);

typedef struct OhPictureHash {
    int32_t  present;                       /* a decoded-picture-hash message was found */
    int32_t  hash_type;                     /* 0 MD5, 1 CRC, 2 checksum */
    uint8_t  md5[3][16];
    uint32_t crc[3];
    uint32_t checksum[3];
} OhPictureHash;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  Walks its messages; a decoded picture hash (payload type 132 in a suffix
 * SEI, 256 in a prefix SEI as the reference also accepts) fills *out.  Returns 1 found, 0 none, -1 malformed / not an SEI NAL unit. */
int oh_sei_picture_hash(const uint8_t *nal, size_t size, OhPictureHash *out);

/* The HDR messages of H.265 Annex D, which the reference does not parse: mastering display colour volume (payload type 137, 24 bytes),
 * content light level information (144, 4 bytes) and alternative transfer characteristics (147, 1 byte); every field big-endian. */
typedef struct OhHdrSei {
    int32_t  has_mastering;
    uint16_t primaries[3][2], white[2];     /* display_primaries_x / _y [c] and white_point_x / _y as coded (units of 0.00002) */
    uint32_t max_lum, min_lum;              /* payload 137; raw units: 0.0001 cd/m2 both (max_lum / 10000 = nits) */
    int32_t  has_cll;
    uint16_t max_cll, max_fall;             /* payload 144: cd/m2; 0 = unknown */
    int32_t  has_alt_transfer;
    int32_t  preferred_transfer;            /* payload 147: preferred_transfer_characteristics (H.273) */
} OhHdrSei;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  The same message walk as oh_sei_picture_hash.  The three messages count
 * in a prefix SEI only (D.2.1); in a suffix SEI they are passed over.  Returns how many of the three kinds were found (0 .. 3; *out is
 * zero where nothing was), or -1: not an SEI NAL unit, a message that runs past the unit, or one of the three with a payload shorter
 * than its fields. */
int oh_sei_hdr(const uint8_t *nal, size_t size, OhHdrSei *out);

/* The display orientation message of H.265 Annex D (payload type 47), which the reference passes over like the HDR messages: how the
 * decoded picture is meant to be flipped and turned for display.  Bits, MSB first: display_orientation_cancel_flag u(1); unless
 * cancelled hor_flip u(1), ver_flip u(1), anticlockwise_rotation u(16), display_orientation_persistence_flag u(1) — 20 bits, a payload
 * of 3 bytes with its alignment bits; a cancelled message takes 1 byte.  oh_orient_from_sei (ohevc_hip.h) turns the fields into an
 * orientation of oh_pics_orient. */
typedef struct OhDisplayOrientation {
    int32_t  present;                 /* a message was found */
    int32_t  cancel;                  /* display_orientation_cancel_flag; the fields below are 0 then */
    int32_t  hor_flip, ver_flip;
    uint32_t anticlockwise_rotation;  /* u(16), units of 360 / 65536 degrees */
    int32_t  persistence;
} OhDisplayOrientation;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  The same message walk as oh_sei_hdr.  The message counts in a prefix SEI
 * only; in a suffix SEI it is passed over; of several in one unit the last counts.  Returns 1 found, 0 none (*out is zero), or -1: not
 * an SEI NAL unit, a message that runs past the unit, or a display orientation with a payload shorter than its fields. */
int oh_sei_display_orientation(const uint8_t *nal, size_t size, OhDisplayOrientation *out);

/* The picture timing message of H.265 Annex D (payload type 1), of which the reference keeps pic_struct (hevc_sei.c:85-101) to tag its
 * frames interlaced_frame / top_field_first.  With frame_field_info_present_flag set the payload starts, MSB first, with pic_struct
 * u(4), source_scan_type u(2), duplicate_flag u(1); the HRD fields that may follow are not read.  The flag is a VUI field of the SPS:
 * the caller passes it.  Without it the message holds none of the three, and they are -1, the reference's "unknown".
 * oh_field_info (ohevc_hip.h) says what a pic_struct means. */
typedef struct OhPicTiming {
    int32_t present;                  /* a message was found */
    int32_t pic_struct;               /* 0 .. 15 as coded (13 .. 15 are reserved); -1 unknown */
    int32_t source_scan_type;         /* 0 interlaced, 1 progressive, 2 unknown, 3 reserved; -1 unknown */
    int32_t duplicate_flag;           /* -1 unknown */
} OhPicTiming;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  The same message walk as oh_sei_display_orientation.  The message counts
 * in a prefix SEI only; in a suffix SEI it is passed over; of several in one unit the last counts.  Returns 1 found, 0 none (*out is
 * zero), or -1: not an SEI NAL unit, a message that runs past the unit, or frame_field_info_present set and an empty payload. */
int oh_sei_pic_timing(const uint8_t *nal, size_t size, int frame_field_info_present, OhPicTiming *out);

/* The film grain characteristics message of H.265 Annex D (payload type 19), which the reference does not parse: the grain that the
 * encoder removed and the decoder is to synthesise again on the displayed picture.  Bits, MSB first, of the unescaped payload:
 * film_grain_characteristics_cancel_flag u(1); unless cancelled film_grain_model_id u(2), separate_colour_description_present_flag
 * u(1); with the description film_grain_bit_depth_luma_minus8 u(3), film_grain_bit_depth_chroma_minus8 u(3), film_grain_full_range_flag
 * u(1), film_grain_colour_primaries u(8), film_grain_transfer_characteristics u(8), film_grain_matrix_coeffs u(8); then
 * blending_mode_id u(2), log2_scale_factor u(4), comp_model_present_flag[c] u(1) for c = 0 .. 2; per present c
 * num_intensity_intervals_minus1 u(8), num_model_values_minus1 u(3) and per interval intensity_interval_lower_bound u(8),
 * intensity_interval_upper_bound u(8) and per model value comp_model_value se(v); at the end
 * film_grain_characteristics_persistence_flag u(1).  Every field is kept as coded; what lies behind a cancel flag, an absent
 * description or an absent component is 0.  oh_grain_from_sei (ohevc_hip.h) turns the message into the tables of oh_pics_grain. */
enum { OH_FG_MAX_INTERVALS = 256, OH_FG_MAX_VALUES = 6 };
typedef struct OhFilmGrainSei {
    int32_t present;                  /* a message was found */
    int32_t cancel;                   /* film_grain_characteristics_cancel_flag */
    int32_t model_id;
    int32_t separate_colour_description;
    int32_t bit_depth_luma_minus8, bit_depth_chroma_minus8, full_range;
    int32_t colour_primaries, transfer_characteristics, matrix_coeffs;
    int32_t blending_mode_id, log2_scale_factor;
    int32_t comp_model_present[3];
    int32_t num_intensity_intervals_minus1[3], num_model_values_minus1[3];
    int32_t persistence;
    uint8_t lower[3][OH_FG_MAX_INTERVALS], upper[3][OH_FG_MAX_INTERVALS];
    int32_t value[3][OH_FG_MAX_INTERVALS][OH_FG_MAX_VALUES];
} OhFilmGrainSei;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  The same message walk as oh_sei_display_orientation.  The message counts
 * in a prefix SEI only; in a suffix SEI it is passed over; of several in one unit the last counts.  Returns 1 found, 0 none (*out is
 * zero), or -1 (*out is zero): not an SEI NAL unit, a message that runs past the unit, a field that lies past the end of the payload,
 * num_model_values_minus1 above 5, an se(v) code of more than 32 leading zeros or one whose value does not fit an int32_t. */
int oh_sei_film_grain(const uint8_t *nal, size_t size, OhFilmGrainSei *out);

/* The colour remapping information message of H.265 Annex D (payload type 142), which the reference does not parse: how a display is
 * to turn the decoded pictures into the rendition that the content owner graded — a piecewise-linear table per component, a 3 x 3
 * matrix, a second table per component.  Bits, MSB first, of the unescaped payload: colour_remap_id ue(v), colour_remap_cancel_flag
 * u(1); unless cancelled colour_remap_persistence_flag u(1), colour_remap_video_signal_info_present_flag u(1); with the signal info
 * colour_remap_full_range_flag u(1), colour_remap_primaries u(8), colour_remap_transfer_function u(8),
 * colour_remap_matrix_coefficients u(8); then colour_remap_input_bit_depth u(8), colour_remap_output_bit_depth u(8); for c = 0 .. 2
 * pre_lut_num_val_minus1[c] u(8) and, where that is above 0, for i = 0 .. pre_lut_num_val_minus1[c] pre_lut_coded_value[c][i] u(vi),
 * pre_lut_target_value[c][i] u(vo); colour_remap_matrix_present_flag u(1); with the matrix log2_matrix_denom u(4) and
 * colour_remap_coeffs[c][i] se(v) for c, i = 0 .. 2; for c = 0 .. 2 post_lut_num_val_minus1[c] u(8) and, where that is above 0, per i
 * post_lut_coded_value[c][i] u(vo), post_lut_target_value[c][i] u(vo).  The widths: vi = ((input_bit_depth + 7) >> 3) << 3, vo the
 * same of output_bit_depth.  Every field is kept as coded; what lies behind a cancel flag or an absent flag is 0.  oh_remap_from_sei
 * (ohevc_hip.h) turns the message into what oh_pics_colour_remap takes. */
enum { OH_CRI_MAX_PIVOTS = 33 };
typedef struct OhColourRemapSei {
    int32_t present;                  /* a message was found */
    int32_t cancel;                   /* colour_remap_cancel_flag */
    uint32_t id;                      /* colour_remap_id */
    int32_t persistence;
    int32_t video_signal_info_present, full_range, primaries, transfer_function, matrix_coefficients;
    int32_t input_bit_depth, output_bit_depth;
    int32_t pre_lut_num_val_minus1[3];
    uint16_t pre_lut_coded_value[3][OH_CRI_MAX_PIVOTS], pre_lut_target_value[3][OH_CRI_MAX_PIVOTS];
    int32_t matrix_present, log2_matrix_denom;
    int32_t coeffs[3][3];
    int32_t post_lut_num_val_minus1[3];
    uint16_t post_lut_coded_value[3][OH_CRI_MAX_PIVOTS], post_lut_target_value[3][OH_CRI_MAX_PIVOTS];
} OhColourRemapSei;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  The same message walk as oh_sei_film_grain.  The message counts in a
 * prefix SEI only; in a suffix SEI it is passed over.  id -1: the last message of the unit counts; otherwise the last one whose
 * colour_remap_id equals id (a stream may carry one message per target display).  Returns 1 found, 0 none (*out is zero), or -1 (*out
 * is zero): not an SEI NAL unit, a message that runs past the unit, a field that lies past the end of the payload, a bit depth outside
 * 8 .. 16 (the widths of the fields behind it are defined only there), a num_val_minus1 above 32, a ue(v) / se(v) code of more than 32
 * leading zeros or one whose value does not fit its type — in any colour remapping message of the unit, selected or not. */
int oh_sei_colour_remap(const uint8_t *nal, size_t size, int64_t id, OhColourRemapSei *out);

/* The frame packing arrangement message (payload type 45): the picture holds the two views of a stereo pair — side by side, one above
 * the other, or one after the other in time.  The layout is the one the reference walks (decode_nal_sei_frame_packing_arrangement,
 * hevc_sei.c:52-75; it keeps arrangement_type, quincunx_sampling_flag and content_interpretation_type and skips the rest).  Bits, MSB
 * first, of the unescaped payload: frame_packing_arrangement_id ue(v), cancel_flag u(1); unless cancelled arrangement_type u(7),
 * quincunx_sampling_flag u(1), content_interpretation_type u(6), spatial_flipping_flag, frame0_flipped_flag, field_views_flag,
 * current_frame_is_frame0_flag, frame0_self_contained_flag, frame1_self_contained_flag u(1) each; only where quincunx_sampling_flag is
 * 0 and arrangement_type is not 5 frame0_grid_position_x, frame0_grid_position_y, frame1_grid_position_x, frame1_grid_position_y
 * u(4) each; reserved_byte u(8), persistence_flag u(1); then, cancelled or not, upsampled_aspect_ratio_flag u(1).  Every field is kept
 * as coded; what lies behind the cancel flag, and grid positions that are not coded, are 0.  oh_packing_from_sei (ohevc_hip.h) turns
 * the message into what oh_pics_unpack / oh_pics_pack take. */
typedef struct OhFramePackingSei {
    int32_t present;                  /* a message was found */
    int32_t cancel;                   /* frame_packing_arrangement_cancel_flag */
    uint32_t id;                      /* frame_packing_arrangement_id */
    int32_t arrangement_type;         /* 3 side by side, 4 top-bottom, 5 temporal interleaving */
    int32_t quincunx_sampling;
    int32_t content_interpretation_type;      /* 0 unspecified, 1 frame 0 is the left view, 2 frame 0 is the right view */
    int32_t spatial_flipping, frame0_flipped, field_views, current_frame_is_frame0, frame0_self_contained, frame1_self_contained;
    int32_t frame0_grid_position_x, frame0_grid_position_y, frame1_grid_position_x, frame1_grid_position_y;
    int32_t reserved_byte;
    int32_t persistence;
    int32_t upsampled_aspect_ratio;
} OhFramePackingSei;
/* nal[0 .. size): one (escaped) SEI NAL unit, header first.  The same message walk as oh_sei_colour_remap.  The message counts in a
 * prefix SEI only; in a suffix SEI it is passed over.  The last message of the unit counts.  Returns 1 found, 0 none (*out is zero),
 * or -1 (*out is zero): not an SEI NAL unit, a message that runs past the unit, a field that lies past the end of the payload, a
 * ue(v) code of more than 32 leading zeros or one whose value does not fit 32 bits — in any frame packing message of the unit. */
int oh_sei_frame_packing(const uint8_t *nal, size_t size, OhFramePackingSei *out);

#ifdef __cplusplus
}
#endif
#endif
