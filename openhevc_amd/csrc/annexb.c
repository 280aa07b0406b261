/*
 * annexb.c — Annex-B byte stream: access-unit splitter, NAL scan, NAL unescape, picture-hash SEI, HDR SEIs, display-orientation, picture timing, film grain, colour remapping and frame packing SEIs.  See include/ohevc_annexb.h for the
 * reference lines each entry point follows.  Plain C, no dependencies.
 */
#include "../../include/ohevc_annexb.h"
#include <stdlib.h>
#include <string.h>

enum { NAL_RASL_R = 9, NAL_BLA_W_LP = 16, NAL_CRA_NUT = 21, NAL_VPS = 32, NAL_AUD = 35, NAL_SEI_PREFIX = 39, NAL_SEI_SUFFIX = 40 };

void oh_au_scanner_init(OhAuScanner *sc)
{
    sc->state64 = ~(uint64_t)0;                               /* no start code in the history */
    sc->frame_start_found = 0;
    sc->reserved = 0;
}

static int is_vcl(int nut) { return nut <= NAL_RASL_R || (nut >= NAL_BLA_W_LP && nut <= NAL_CRA_NUT); }

/* what a NAL unit type means for the access-unit boundary (7.4.2.4.4: the first of VPS .. AUD, prefix SEI, the reserved / unspecified ranges
 * 41..44 and 48..55 after the last VCL NAL unit of a picture starts a new access unit; a VCL NAL unit does when it is a first slice segment) */
enum { CLS_NEUTRAL = 0, CLS_OPENS_AU = 1, CLS_VCL = 2 };
static int nal_class(int nut)
{
    static uint8_t cls[64];
    static int built;
    if (!built) {                                             /* (idempotent: concurrent first calls write the same values) */
        for (int t = 0; t < 64; t++)
            cls[t] = is_vcl(t) ? CLS_VCL : ((t >= NAL_VPS && t <= NAL_AUD) || t == NAL_SEI_PREFIX || (t >= 41 && t <= 44) || (t >= 48 && t <= 55)) ? CLS_OPENS_AU : CLS_NEUTRAL;
        built = 1;
    }
    return cls[nut & 63];
}

/* one NAL unit header seen by the scanner: returns 1 when the access unit that was open ENDS in front of this unit.  Only units of the base
 * layer move the state (hevc_parser.c:62, 71): the pictures of higher layers belong to the access unit of their base-layer picture. */
static int au_step(OhAuScanner *sc, int cls, int layer_id, int first_slice_segment)
{
    if (layer_id != 0 || cls == CLS_NEUTRAL || (cls == CLS_VCL && !first_slice_segment))
        return 0;
    if (!sc->frame_start_found) {                             /* no picture open: a first slice segment opens one, anything else waits */
        sc->frame_start_found = cls == CLS_VCL;
        return 0;
    }
    sc->frame_start_found = 0;                                /* a picture was open: this unit belongs to the next access unit */
    return 1;
}

long oh_au_find_frame_end(OhAuScanner *sc, const uint8_t *buf, size_t size)
{
    /* the history holds the last eight bytes across calls (the parser's state64): a header is complete when the byte BEHIND its two bytes
     * arrives — that byte carries first_slice_segment_in_pic_flag — i.e. when bytes -5 .. -3 of the history are the start code 00 00 01 */
    uint64_t hist = sc->state64;
    for (size_t i = 0; i < size; i++) {
        hist = (hist << 8) | buf[i];
        if ((hist & 0xFFFFFF000000ull) != 0x000001000000ull)
            continue;
        const unsigned h0 = (unsigned)(hist >> 16) & 0xFF, h1 = (unsigned)(hist >> 8) & 0xFF;      /* the two header bytes */
        if (au_step(sc, nal_class((int)(h0 >> 1) & 0x3F), (int)((h0 & 1) << 5 | h1 >> 3), buf[i] >> 7)) {
            sc->state64 = hist;
            return (long)i - 5;                               /* the cut lies in front of the start code (three bytes) + header (two) */
        }
    }
    sc->state64 = hist;
    return OH_AU_END_NOT_FOUND;
}

long oh_annexb_split(const uint8_t *data, size_t size, size_t *offsets, size_t cap)
{
    OhAuScanner sc;
    oh_au_scanner_init(&sc);
    size_t n = 0, pos = 0;
    if (cap > 0) offsets[0] = 0;
    while (pos < size) {
        const long r = oh_au_find_frame_end(&sc, data + pos, size - pos);
        if (r == OH_AU_END_NOT_FOUND)
            break;
        /* the bytes from the cut on are fed again with a fresh history, as the parser's caller re-feeds what ff_combine_frame
         * (parser.c) held back: the start code that closed the access unit is seen once more with frame_start_found = 0, where a
         * parameter set does nothing and a first slice segment opens the next picture */
        pos += (size_t)r;                                     /* r >= 0: a fresh history cannot end inside earlier bytes */
        n++;
        if (n < cap) offsets[n] = pos;
        oh_au_scanner_init(&sc);
    }
    n++;
    if (n < cap) offsets[n] = size;
    return n + 1 <= cap ? (long)n : -(long)(n + 1);
}

long oh_annexb_nal_units(const uint8_t *buf, size_t size, OhNal *out, size_t cap)
{
    size_t pos = 0, n = 0;
    while (size - pos >= 4) {
        if (buf[pos + 2] == 0) {                              /* zero_byte / leading zeros: slide */
            if (buf[pos] != 0) return -1;
            pos++;
            continue;
        }
        if (buf[pos] != 0 || buf[pos + 1] != 0 || buf[pos + 2] != 1)
            return -1;
        pos += 3;
        /* the unit runs to the next 00 00 0x with x < 3 (x == 3 is an escape), or to the end */
        size_t end = size;
        for (size_t i = pos; i + 2 < size; i++)
            if (buf[i] == 0 && buf[i + 1] == 0 && buf[i + 2] < 3) { end = i; break; }
        while (end == size && end > pos + 2 && buf[end - 1] == 0)
            end--, size--;                                    /* trailing_zero_8bits at the end of the buffer (a NAL unit never ends in 00) */
        if (end - pos >= 2 && n < cap) {
            OhNal *u = &out[n];
            u->offset = pos; u->size = end - pos;
            u->type = (buf[pos] >> 1) & 0x3F;
            u->layer_id = ((buf[pos] & 1) << 5) | (buf[pos + 1] >> 3);
            u->temporal_id = (buf[pos + 1] & 7) - 1;
            u->first_slice_segment_in_pic = is_vcl(u->type) && end - pos > 2 ? buf[pos + 2] >> 7 : 0;
        }
        if (end - pos >= 2) n++;
        pos = end;
    }
    return (long)n;
}

long oh_nal_unescape(const uint8_t *src, size_t length, uint8_t *dst, size_t *dst_size, int32_t *skipped_pos, size_t cap, int32_t *n_skipped)
{
    size_t si = 0, di = 0;
    int32_t ns = 0;
    while (si < length) {
        if (si + 2 < length && src[si] == 0 && src[si + 1] == 0 && src[si + 2] <= 3) {
            if (src[si + 2] != 3)
                break;                                        /* next start code: past the end of this unit */
            dst[di++] = 0; dst[di++] = 0;
            si += 3;
            if ((size_t)ns < cap && skipped_pos) skipped_pos[ns] = (int32_t)di - 1;
            ns++;
            continue;
        }
        dst[di++] = src[si++];
    }
    if (dst_size) *dst_size = di;
    if (n_skipped) *n_skipped = ns;
    return (long)si;
}

/* The message walk both SEI readers share: nal[0 .. size) is one (escaped) SEI NAL unit, header first.  Calls on_msg(ctx, nut,
 * payloadType, payload, payloadSize) for every sei_message(); on_msg returns -1 for a payload it cannot accept.  Returns 0, or -1: not
 * an SEI NAL unit, a message that runs past the unit, or on_msg said so (the walk stops there). */
typedef int (*SeiMsgFn)(void *ctx, int nut, unsigned type, const uint8_t *payload, unsigned len);
static int sei_walk(const uint8_t *nal, size_t size, SeiMsgFn on_msg, void *ctx)
{
    if (size < 3)
        return -1;
    const int nut = (nal[0] >> 1) & 0x3F;
    if (nut != NAL_SEI_PREFIX && nut != NAL_SEI_SUFFIX)
        return -1;
    uint8_t *rbsp = (uint8_t *)malloc(size);
    if (!rbsp)
        return -1;
    size_t n = 0;
    oh_nal_unescape(nal, size, rbsp, &n, NULL, 0, NULL);
    size_t p = 2;                                             /* behind the NAL header */
    int bad = 0;
    /* sei_message()s until only rbsp_trailing_bits are left (hevc_sei.c:183-200 more_rbsp_data): the LAST byte being 0x80.  A 0x80
     * anywhere else is a payloadType (128, structure_of_pictures_info), not the end: another message may follow it in the same NAL */
    while (n > 0 && rbsp[n - 1] == 0) n--;                    /* cabac_zero_words / trailing zero bytes behind the trailing bits */
    while (p < n && !(p == n - 1 && rbsp[p] == 0x80)) {
        unsigned type = 0, len = 0;
        while (p < n && rbsp[p] == 0xFF) { type += 255; p++; }
        if (p >= n) { bad = 1; break; }
        type += rbsp[p++];
        while (p < n && rbsp[p] == 0xFF) { len += 255; p++; }
        if (p >= n) { bad = 1; break; }
        len += rbsp[p++];
        if (p + len > n) { bad = 1; break; }
        if (on_msg(ctx, nut, type, rbsp + p, len) < 0) { bad = 1; break; }
        p += len;
    }
    free(rbsp);
    return bad ? -1 : 0;
}

static int hash_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    OhPictureHash *out = (OhPictureHash *)ctx;
    if (!((nut == NAL_SEI_SUFFIX && type == 132) || (nut == NAL_SEI_PREFIX && type == 256)))
        return 0;
    if (len < 1)
        return -1;
    const int ht = q[0];
    const unsigned per = ht == 0 ? 16 : ht == 1 ? 2 : ht == 2 ? 4 : 0;
    if (!per || len < 1 + per)
        return -1;
    const unsigned planes = (len - 1) / per < 3 ? (len - 1) / per : 3;      /* monochrome streams carry one */
    out->present = 1;
    out->hash_type = ht;
    for (unsigned c = 0; c < planes; c++) {
        const uint8_t *v = q + 1 + c * per;
        if (ht == 0) memcpy(out->md5[c], v, 16);
        else if (ht == 1) out->crc[c] = ((uint32_t)v[0] << 8) | v[1];
        else out->checksum[c] = ((uint32_t)v[0] << 24) | ((uint32_t)v[1] << 16) | ((uint32_t)v[2] << 8) | v[3];
    }
    return 0;
}

int oh_sei_picture_hash(const uint8_t *nal, size_t size, OhPictureHash *out)
{
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, hash_msg, out) < 0)
        return -1;
    return out->present;
}

static unsigned be16(const uint8_t *v) { return ((unsigned)v[0] << 8) | v[1]; }
static uint32_t be32(const uint8_t *v) { return ((uint32_t)v[0] << 24) | ((uint32_t)v[1] << 16) | ((uint32_t)v[2] << 8) | v[3]; }

static int hdr_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    OhHdrSei *out = (OhHdrSei *)ctx;
    if (nut != NAL_SEI_PREFIX)
        return 0;
    if (type == 137) {                                        /* D.2.28 mastering_display_colour_volume */
        if (len < 24)
            return -1;
        for (int c = 0; c < 3; c++) {
            out->primaries[c][0] = (uint16_t)be16(q + 4 * c);
            out->primaries[c][1] = (uint16_t)be16(q + 4 * c + 2);
        }
        out->white[0] = (uint16_t)be16(q + 12); out->white[1] = (uint16_t)be16(q + 14);
        out->max_lum = be32(q + 16); out->min_lum = be32(q + 20);
        out->has_mastering = 1;
    } else if (type == 144) {                                 /* D.2.35 content_light_level_info */
        if (len < 4)
            return -1;
        out->max_cll = (uint16_t)be16(q); out->max_fall = (uint16_t)be16(q + 2);
        out->has_cll = 1;
    } else if (type == 147) {                                 /* D.2.38 alternative_transfer_characteristics */
        if (len < 1)
            return -1;
        out->preferred_transfer = q[0];
        out->has_alt_transfer = 1;
    }
    return 0;
}

int oh_sei_hdr(const uint8_t *nal, size_t size, OhHdrSei *out)
{
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, hdr_msg, out) < 0) {
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return out->has_mastering + out->has_cll + out->has_alt_transfer;
}

static int disp_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    OhDisplayOrientation *out = (OhDisplayOrientation *)ctx;
    if (nut != NAL_SEI_PREFIX || type != 47)                  /* D.2.17 display_orientation */
        return 0;
    if (len < 1)
        return -1;
    memset(out, 0, sizeof(*out));                             /* the last message of the unit counts */
    out->present = 1;
    out->cancel = q[0] >> 7;
    if (out->cancel)
        return 0;
    if (len < 3)                                              /* cancel, two flips, u(16), persistence: 20 bits */
        return -1;
    const uint32_t bits = ((uint32_t)q[0] << 16) | ((uint32_t)q[1] << 8) | q[2];
    out->hor_flip = (bits >> 22) & 1;
    out->ver_flip = (bits >> 21) & 1;
    out->anticlockwise_rotation = (bits >> 5) & 0xFFFF;
    out->persistence = (bits >> 4) & 1;
    return 0;
}

int oh_sei_display_orientation(const uint8_t *nal, size_t size, OhDisplayOrientation *out)
{
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, disp_msg, out) < 0) {
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return out->present;
}

struct timing_ctx { OhPicTiming *out; int info_present; };

static int timing_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    struct timing_ctx *t = (struct timing_ctx *)ctx;
    OhPicTiming *out = t->out;
    if (nut != NAL_SEI_PREFIX || type != 1)                   /* D.2.3 pic_timing */
        return 0;
    memset(out, 0, sizeof(*out));                             /* the last message of the unit counts */
    out->present = 1;
    out->pic_struct = out->source_scan_type = out->duplicate_flag = -1;     /* unknown without frame_field_info_present_flag */
    if (!t->info_present)
        return 0;
    if (len < 1)                                              /* pic_struct u(4), source_scan_type u(2), duplicate_flag u(1) */
        return -1;
    out->pic_struct = q[0] >> 4;
    out->source_scan_type = (q[0] >> 2) & 3;
    out->duplicate_flag = (q[0] >> 1) & 1;
    return 0;
}

int oh_sei_pic_timing(const uint8_t *nal, size_t size, int frame_field_info_present, OhPicTiming *out)
{
    struct timing_ctx t = { out, frame_field_info_present != 0 };
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, timing_msg, &t) < 0) {
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return out->present;
}

/* bits of a payload, MSB first; a read past the end sets bad and gives 0 */
struct bit_reader { const uint8_t *p; size_t bits, at; int bad; };

static uint32_t get_bits(struct bit_reader *b, int n)       /* n in 0 .. 32 */
{
    uint32_t v = 0;
    if (b->bad || (size_t)n > b->bits - b->at) {
        b->bad = 1;
        return 0;
    }
    for (int i = 0; i < n; i++, b->at++)
        v = (v << 1) | ((b->p[b->at >> 3] >> (7 - (b->at & 7))) & 1);
    return v;
}

/* se(v) of H.265 9.2: codeNum k = 2^z - 1 + the z bits behind the z leading zeros and the one; the value is (k + 1) / 2 for an odd k
 * and -k / 2 for an even one */
static int32_t get_se(struct bit_reader *b)
{
    int z = 0;
    while (!b->bad && !get_bits(b, 1))
        if (++z > 32)
            b->bad = 1;
    if (b->bad)
        return 0;
    const uint64_t k = (((uint64_t)1 << z) - 1) + get_bits(b, z);
    const int64_t v = (k & 1) ? (int64_t)((k + 1) >> 1) : -(int64_t)(k >> 1);
    if (b->bad || v > INT32_MAX || v < INT32_MIN) {
        b->bad = 1;
        return 0;
    }
    return (int32_t)v;
}

static int grain_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    OhFilmGrainSei *out = (OhFilmGrainSei *)ctx;
    if (nut != NAL_SEI_PREFIX || type != 19)                  /* D.2.21 film_grain_characteristics */
        return 0;
    struct bit_reader b = { q, (size_t)len * 8, 0, 0 };
    memset(out, 0, sizeof(*out));                             /* the last message of the unit counts */
    out->present = 1;
    out->cancel = (int32_t)get_bits(&b, 1);
    if (b.bad)
        return -1;
    if (out->cancel)
        return 0;
    out->model_id = (int32_t)get_bits(&b, 2);
    out->separate_colour_description = (int32_t)get_bits(&b, 1);
    if (out->separate_colour_description) {
        out->bit_depth_luma_minus8 = (int32_t)get_bits(&b, 3);
        out->bit_depth_chroma_minus8 = (int32_t)get_bits(&b, 3);
        out->full_range = (int32_t)get_bits(&b, 1);
        out->colour_primaries = (int32_t)get_bits(&b, 8);
        out->transfer_characteristics = (int32_t)get_bits(&b, 8);
        out->matrix_coeffs = (int32_t)get_bits(&b, 8);
    }
    out->blending_mode_id = (int32_t)get_bits(&b, 2);
    out->log2_scale_factor = (int32_t)get_bits(&b, 4);
    for (int c = 0; c < 3; c++)
        out->comp_model_present[c] = (int32_t)get_bits(&b, 1);
    for (int c = 0; c < 3 && !b.bad; c++) {
        if (!out->comp_model_present[c])
            continue;
        out->num_intensity_intervals_minus1[c] = (int32_t)get_bits(&b, 8);
        out->num_model_values_minus1[c] = (int32_t)get_bits(&b, 3);
        if (b.bad || out->num_model_values_minus1[c] >= OH_FG_MAX_VALUES)
            return -1;
        for (int i = 0; i <= out->num_intensity_intervals_minus1[c] && !b.bad; i++) {
            out->lower[c][i] = (uint8_t)get_bits(&b, 8);
            out->upper[c][i] = (uint8_t)get_bits(&b, 8);
            for (int j = 0; j <= out->num_model_values_minus1[c]; j++)
                out->value[c][i][j] = get_se(&b);
        }
    }
    out->persistence = (int32_t)get_bits(&b, 1);
    return b.bad ? -1 : 0;
}

int oh_sei_film_grain(const uint8_t *nal, size_t size, OhFilmGrainSei *out)
{
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, grain_msg, out) < 0) {
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return out->present;
}

/* ue(v) of H.265 9.2: codeNum 2^z - 1 + the z bits behind the z leading zeros and the one */
static uint32_t get_ue(struct bit_reader *b)
{
    int z = 0;
    while (!b->bad && !get_bits(b, 1))
        if (++z > 32)
            b->bad = 1;
    if (b->bad)
        return 0;
    const uint64_t k = (((uint64_t)1 << z) - 1) + get_bits(b, z);
    if (b->bad || k > UINT32_MAX) {
        b->bad = 1;
        return 0;
    }
    return (uint32_t)k;
}

/* num_val_minus1 and, where it is above 0, the pivots of one curve of the colour remapping message: coded values of vc bits, target
 * values of vt bits */
static void remap_curve_fields(struct bit_reader *b, int vc, int vt, int32_t *num_val_minus1, uint16_t *coded, uint16_t *target)
{
    *num_val_minus1 = (int32_t)get_bits(b, 8);
    if (*num_val_minus1 >= OH_CRI_MAX_PIVOTS) {
        b->bad = 1;
        return;
    }
    if (*num_val_minus1 > 0)
        for (int i = 0; i <= *num_val_minus1 && !b->bad; i++) {
            coded[i] = (uint16_t)get_bits(b, vc);
            target[i] = (uint16_t)get_bits(b, vt);
        }
}

struct remap_ctx { OhColourRemapSei *out; int64_t id; };

static int remap_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    struct remap_ctx *r = (struct remap_ctx *)ctx;
    if (nut != NAL_SEI_PREFIX || type != 142)                 /* D.2.33 colour_remapping_info */
        return 0;
    struct bit_reader b = { q, (size_t)len * 8, 0, 0 };
    OhColourRemapSei m;
    memset(&m, 0, sizeof(m));
    m.present = 1;
    m.id = get_ue(&b);
    m.cancel = (int32_t)get_bits(&b, 1);
    if (b.bad)
        return -1;
    if (!m.cancel) {
        m.persistence = (int32_t)get_bits(&b, 1);
        m.video_signal_info_present = (int32_t)get_bits(&b, 1);
        if (m.video_signal_info_present) {
            m.full_range = (int32_t)get_bits(&b, 1);
            m.primaries = (int32_t)get_bits(&b, 8);
            m.transfer_function = (int32_t)get_bits(&b, 8);
            m.matrix_coefficients = (int32_t)get_bits(&b, 8);
        }
        m.input_bit_depth = (int32_t)get_bits(&b, 8);
        m.output_bit_depth = (int32_t)get_bits(&b, 8);
        if (b.bad || m.input_bit_depth < 8 || m.input_bit_depth > 16 || m.output_bit_depth < 8 || m.output_bit_depth > 16)
            return -1;
        const int vi = ((m.input_bit_depth + 7) >> 3) << 3, vo = ((m.output_bit_depth + 7) >> 3) << 3;
        for (int c = 0; c < 3 && !b.bad; c++)
            remap_curve_fields(&b, vi, vo, &m.pre_lut_num_val_minus1[c], m.pre_lut_coded_value[c], m.pre_lut_target_value[c]);
        m.matrix_present = (int32_t)get_bits(&b, 1);
        if (m.matrix_present) {
            m.log2_matrix_denom = (int32_t)get_bits(&b, 4);
            for (int c = 0; c < 3; c++)
                for (int i = 0; i < 3; i++)
                    m.coeffs[c][i] = get_se(&b);
        }
        for (int c = 0; c < 3 && !b.bad; c++)
            remap_curve_fields(&b, vo, vo, &m.post_lut_num_val_minus1[c], m.post_lut_coded_value[c], m.post_lut_target_value[c]);
        if (b.bad)
            return -1;
    }
    if (r->id < 0 || (int64_t)m.id == r->id)                  /* the last one that is asked for counts */
        *r->out = m;
    return 0;
}

int oh_sei_colour_remap(const uint8_t *nal, size_t size, int64_t id, OhColourRemapSei *out)
{
    struct remap_ctx r = { out, id };
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, remap_msg, &r) < 0) {
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return out->present;
}

static int packing_msg(void *ctx, int nut, unsigned type, const uint8_t *q, unsigned len)
{
    OhFramePackingSei *out = (OhFramePackingSei *)ctx;
    if (nut != NAL_SEI_PREFIX || type != 45)                  /* D.2.16 frame_packing_arrangement, as hevc_sei.c:52-75 walks it */
        return 0;
    struct bit_reader b = { q, (size_t)len * 8, 0, 0 };
    OhFramePackingSei m;
    memset(&m, 0, sizeof(m));
    m.present = 1;
    m.id = get_ue(&b);
    m.cancel = (int32_t)get_bits(&b, 1);
    if (!m.cancel) {
        m.arrangement_type = (int32_t)get_bits(&b, 7);
        m.quincunx_sampling = (int32_t)get_bits(&b, 1);
        m.content_interpretation_type = (int32_t)get_bits(&b, 6);
        m.spatial_flipping = (int32_t)get_bits(&b, 1);
        m.frame0_flipped = (int32_t)get_bits(&b, 1);
        m.field_views = (int32_t)get_bits(&b, 1);
        m.current_frame_is_frame0 = (int32_t)get_bits(&b, 1);
        m.frame0_self_contained = (int32_t)get_bits(&b, 1);
        m.frame1_self_contained = (int32_t)get_bits(&b, 1);
        if (!m.quincunx_sampling && m.arrangement_type != 5) {
            m.frame0_grid_position_x = (int32_t)get_bits(&b, 4);
            m.frame0_grid_position_y = (int32_t)get_bits(&b, 4);
            m.frame1_grid_position_x = (int32_t)get_bits(&b, 4);
            m.frame1_grid_position_y = (int32_t)get_bits(&b, 4);
        }
        m.reserved_byte = (int32_t)get_bits(&b, 8);
        m.persistence = (int32_t)get_bits(&b, 1);
    }
    m.upsampled_aspect_ratio = (int32_t)get_bits(&b, 1);
    if (b.bad)
        return -1;
    *out = m;                                                 /* the last message of the unit counts */
    return 0;
}

int oh_sei_frame_packing(const uint8_t *nal, size_t size, OhFramePackingSei *out)
{
    memset(out, 0, sizeof(*out));
    if (sei_walk(nal, size, packing_msg, out) < 0) {
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return out->present;
}
