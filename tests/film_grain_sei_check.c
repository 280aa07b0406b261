/* film_grain_sei_check.c — the film grain SEI reader (openhevc_amd/csrc/annexb.c: oh_sei_film_grain) run on the CPU as a program of its
 * own; built together with that file, with AddressSanitizer and UBSan, by tests/test_film_grain_sei_host.py.  Every NAL unit is a heap
 * block of exactly its size, so a read one byte past the unit is a sanitizer report; the units are written by a bit writer here: the
 * largest message (three components of 256 intervals and six model values of 32 leading zeros each), messages at every truncation of
 * the unit and of the payload, a payload that needs emulation-prevention bytes, and payloads of every byte value.  Exit status 0: every
 * check held. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/ohevc_annexb.h"

static int failures;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            failures++;                                                                    \
            fprintf(stderr, "%s (line %d): ", #cond, __LINE__);                             \
            fprintf(stderr, __VA_ARGS__);                                                  \
            fprintf(stderr, "\n");                                                         \
        }                                                                                  \
    } while (0)

struct bits { uint8_t *p; size_t n, cap; };                   /* n: bits written */

static void put(struct bits *b, int n, uint64_t v)
{
    for (int i = n - 1; i >= 0; i--, b->n++) {
        if (b->n / 8 >= b->cap) {
            b->cap = b->cap ? 2 * b->cap : 64;
            b->p = (uint8_t *)realloc(b->p, b->cap);
            memset(b->p + b->n / 8, 0, b->cap - b->n / 8);
        }
        if ((v >> i) & 1)
            b->p[b->n / 8] |= (uint8_t)(0x80 >> (b->n & 7));
    }
}

static void put_se(struct bits *b, int64_t v)
{
    const uint64_t k = v > 0 ? 2 * (uint64_t)v - 1 : 2 * (uint64_t)-v;
    int z = 0;
    while (((k + 1) >> (z + 1)) != 0) z++;
    put(b, z, 0);
    put(b, 1, 1);
    put(b, z, (k + 1) - ((uint64_t)1 << z));
}

/* a prefix SEI NAL unit with one film grain message of that payload, escaped, in a heap block of exactly its size */
static uint8_t *unit(const uint8_t *payload, size_t len, size_t *size, int nut)
{
    uint8_t *raw = (uint8_t *)malloc(len + len / 255 + 8), *out;
    size_t n = 0, m = 0, zeros = 0, rest = len;
    raw[n++] = 19;
    for (; rest >= 255; rest -= 255) raw[n++] = 0xFF;
    raw[n++] = (uint8_t)rest;
    memcpy(raw + n, payload, len);
    n += len;
    raw[n++] = 0x80;
    out = (uint8_t *)malloc(2 + n + n / 2 + 1);
    out[m++] = (uint8_t)(nut << 1); out[m++] = 1;
    for (size_t i = 0; i < n; i++) {
        if (zeros >= 2 && raw[i] <= 3) { out[m++] = 3; zeros = 0; }
        out[m++] = raw[i];
        zeros = raw[i] ? 0 : zeros + 1;
    }
    free(raw);
    uint8_t *exact = (uint8_t *)malloc(m ? m : 1);
    memcpy(exact, out, m);
    free(out);
    *size = m;
    return exact;
}

static int read_copy(const uint8_t *nal, size_t size, OhFilmGrainSei *g)
{
    uint8_t *exact = (uint8_t *)malloc(size ? size : 1);       /* the truncated unit in a block of its own */
    memcpy(exact, nal, size);
    const int rc = oh_sei_film_grain(exact, size, g);
    free(exact);
    return rc;
}

static int all_zero(const OhFilmGrainSei *g)
{
    const uint8_t *p = (const uint8_t *)g;
    for (size_t i = 0; i < sizeof(*g); i++)
        if (p[i]) return 0;
    return 1;
}

/* the message: header without (desc 0) or with the colour description, then nc components of ni intervals and nv values each */
static int64_t value_of(int64_t value, int j) { return (j & 1) && value != INT32_MIN ? -value : value; }

static void message(struct bits *b, int desc, int nc, int ni, int nv, int64_t value, int zero_bounds)
{
    put(b, 1, 0); put(b, 2, 0); put(b, 1, (uint64_t)desc);
    if (desc) { put(b, 3, 2); put(b, 3, 4); put(b, 1, 1); put(b, 8, 9); put(b, 8, 16); put(b, 8, 255); }
    put(b, 2, 1); put(b, 4, 15);
    for (int c = 0; c < 3; c++) put(b, 1, c < nc);
    for (int c = 0; c < nc; c++) {
        put(b, 8, (uint64_t)(ni - 1)); put(b, 3, (uint64_t)(nv - 1));
        for (int i = 0; i < ni; i++) {
            put(b, 8, zero_bounds ? 0 : (uint64_t)(i & 255)); put(b, 8, zero_bounds ? 0 : (uint64_t)(255 - (i & 255)));
            for (int j = 0; j < nv; j++) put_se(b, value_of(value, j));
        }
    }
    put(b, 1, 1);
}

static long whole_and_truncated(int desc, int nc, int ni, int nv, int64_t value, int zero_bounds, int every)
{
    long calls = 0;
    struct bits b = { NULL, 0, 0 };
    message(&b, desc, nc, ni, nv, value, zero_bounds);
    const size_t field_bits = b.n;
    put(&b, 1, 1);                                             /* the alignment bits */
    const size_t len = (b.n + 7) / 8;
    size_t size;
    uint8_t *nal = unit(b.p, len, &size, 39);
    OhFilmGrainSei *g = (OhFilmGrainSei *)malloc(sizeof(OhFilmGrainSei));
    if (zero_bounds) {
        int escapes = 0;
        for (size_t i = 2; i + 2 < size; i++)
            escapes += !nal[i] && !nal[i + 1] && nal[i + 2] == 3;
        CHECK(escapes >= ni, "%d emulation-prevention bytes", escapes);
    }
    CHECK(read_copy(nal, size, g) == 1, "the whole unit (%d components, %d intervals, %d values)", nc, ni, nv);
    CHECK(g->present == 1 && !g->cancel && g->separate_colour_description == desc && g->blending_mode_id == 1 && g->log2_scale_factor == 15 &&
          g->persistence == 1, "head");
    CHECK(!desc || (g->bit_depth_luma_minus8 == 2 && g->bit_depth_chroma_minus8 == 4 && g->full_range == 1 && g->colour_primaries == 9 &&
                    g->transfer_characteristics == 16 && g->matrix_coeffs == 255), "colour description");
    for (int c = 0; c < 3; c++) {
        CHECK(g->comp_model_present[c] == (c < nc), "component %d", c);
        if (c >= nc) continue;
        CHECK(g->num_intensity_intervals_minus1[c] == ni - 1 && g->num_model_values_minus1[c] == nv - 1, "counts of component %d", c);
        for (int i = 0; i < ni; i++) {
            CHECK(g->lower[c][i] == (zero_bounds ? 0 : i & 255) && g->upper[c][i] == (zero_bounds ? 0 : 255 - (i & 255)), "bounds [%d][%d]", c, i);
            for (int j = 0; j < OH_FG_MAX_VALUES; j++)
                CHECK(g->value[c][i][j] == (j >= nv ? 0 : value_of(value, j)), "value [%d][%d][%d] = %d", c, i, j, g->value[c][i][j]);
        }
    }
    calls++;
    /* the unit cut to every shorter length (or to `every`-th) that cuts the message: without its last byte, the trailing bits, the
     * message is still whole */
    for (size_t k = 0; k + 1 < size; k += (size_t)every) {
        const int rc = read_copy(nal, k, g);
        CHECK(rc == -1 && all_zero(g), "unit cut to %zu of %zu bytes: %d", k, size, rc);
        calls++;
    }
    free(nal);
    /* the payload cut to every shorter length, the unit whole around it */
    CHECK(field_bits % 8 != 0, "the last byte holds a field");
    for (size_t k = 0; k < len; k += (size_t)every) {
        nal = unit(b.p, k, &size, 39);
        const int rc = read_copy(nal, size, g);
        CHECK(rc == -1 && all_zero(g), "payload cut to %zu of %zu bytes: %d", k, len, rc);
        free(nal);
        calls++;
    }
    /* in a suffix SEI it is passed over */
    nal = unit(b.p, len, &size, 40);
    CHECK(read_copy(nal, size, g) == 0 && all_zero(g), "suffix SEI");
    free(nal);
    free(g);
    free(b.p);
    return calls + 1;
}

/* payloads of 1 .. 4 bytes of every value of the first two bytes, and pseudo-random longer ones: any answer, no report */
static long arbitrary(void)
{
    long calls = 0;
    OhFilmGrainSei *g = (OhFilmGrainSei *)malloc(sizeof(OhFilmGrainSei));
    uint8_t p[64];
    uint32_t x = 19;
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b += 5)
            for (size_t len = 1; len <= 4; len++) {
                size_t size;
                p[0] = (uint8_t)a; p[1] = (uint8_t)b; p[2] = (uint8_t)(a ^ b); p[3] = 0;
                uint8_t *nal = unit(p, len, &size, 39);
                const int rc = read_copy(nal, size, g);
                CHECK(rc == 1 || (rc == -1 && all_zero(g)), "arbitrary payload: %d", rc);
                free(nal);
                calls++;
            }
    for (int t = 0; t < 4000; t++) {
        size_t size;
        const size_t len = 1 + t % 64;
        for (size_t i = 0; i < len; i++) { x = x * 1664525u + 1013904223u; p[i] = (uint8_t)(x >> 24) & (t & 1 ? 0xFF : 0x11); }
        p[0] &= 0x7F;                                          /* not cancelled */
        uint8_t *nal = unit(p, len, &size, 39);
        const int rc = read_copy(nal, size, g);
        CHECK(rc == 1 || (rc == -1 && all_zero(g)), "pseudo-random payload: %d", rc);
        free(nal);
        calls++;
    }
    free(g);
    return calls;
}

int main(void)
{
    printf("small messages at every truncation: %ld calls\n",
           whole_and_truncated(0, 1, 1, 1, 1, 0, 1) + whole_and_truncated(1, 3, 3, 3, 100, 0, 1) + whole_and_truncated(0, 2, 2, 6, -70000, 0, 1));
    /* bounds 0 / 0 byte aligned behind 24 bits of head, then se(32) = 000000 1000000: 00 00 02 needs an emulation-prevention byte */
    printf("zero runs (emulation prevention) at every truncation: %ld calls\n", whole_and_truncated(0, 1, 1, 1, 32, 1, 1) + whole_and_truncated(0, 3, 8, 1, 32, 1, 1));
    printf("the largest message, every 97th truncation: %ld calls\n", whole_and_truncated(1, 3, 256, 6, INT32_MIN, 0, 97));
    printf("arbitrary payloads: %ld calls\n", arbitrary());
    if (failures) {
        printf("film grain sei: %d checks failed\n", failures);
        return 1;
    }
    printf("film grain sei ok\n");
    return 0;
}
