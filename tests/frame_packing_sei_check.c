/* frame_packing_sei_check.c — the frame packing arrangement SEI reader (openhevc_amd/csrc/annexb.c: oh_sei_frame_packing) run on the CPU
 * as a program of its own; built together with that file, with AddressSanitizer and UBSan, by tests/test_frame_packing_sei_host.py.
 * Every NAL unit is a heap block of exactly its size, so a read one byte past the unit is a sanitizer report; the units are written by
 * a bit writer here: every arrangement type with every flag pattern, the longest id, messages at every truncation of the unit and of
 * the payload, a payload that needs emulation-prevention bytes, two messages in one unit, and payloads of every byte value.  Exit
 * status 0: every check held. */
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

static void put_ue(struct bits *b, uint64_t k)
{
    int z = 0;
    while (((k + 1) >> (z + 1)) != 0) z++;
    put(b, z, 0);
    put(b, 1, 1);
    put(b, z, (k + 1) - ((uint64_t)1 << z));
}

/* an SEI NAL unit of nm messages of type 45 with those payloads, escaped, in a heap block of exactly its size */
static uint8_t *unit(const uint8_t *const payload[], const size_t len[], int nm, size_t *size, int nut)
{
    size_t total = 8, n = 0, m = 0, zeros = 0;
    for (int k = 0; k < nm; k++) total += len[k] + len[k] / 255 + 4;
    uint8_t *raw = (uint8_t *)malloc(total), *out;
    for (int k = 0; k < nm; k++) {
        size_t rest = len[k];
        raw[n++] = 45;
        for (; rest >= 255; rest -= 255) raw[n++] = 0xFF;
        raw[n++] = (uint8_t)rest;
        if (len[k]) memcpy(raw + n, payload[k], len[k]);
        n += len[k];
    }
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

static uint8_t *unit1(const uint8_t *payload, size_t len, size_t *size, int nut) { return unit(&payload, &len, 1, size, nut); }

static int read_copy(const uint8_t *nal, size_t size, OhFramePackingSei *r)
{
    uint8_t *exact = (uint8_t *)malloc(size ? size : 1);       /* the truncated unit in a block of its own */
    memcpy(exact, nal, size);
    const int rc = oh_sei_frame_packing(exact, size, r);
    free(exact);
    return rc;
}

static int all_zero(const OhFramePackingSei *r)
{
    const uint8_t *p = (const uint8_t *)r;
    for (size_t i = 0; i < sizeof(*r); i++)
        if (p[i]) return 0;
    return 1;
}

/* the message: id, type, quincunx, the six flags as the bits of `flags` (spatial_flipping the highest), grid positions g, 2 g, 3 g, 4 g mod 16 */
static void message(struct bits *b, uint64_t id, int type, int quincunx, int cit, int flags, int g, int reserved, int persistence, int uar)
{
    put_ue(b, id); put(b, 1, 0);
    put(b, 7, (uint64_t)type); put(b, 1, (uint64_t)quincunx); put(b, 6, (uint64_t)cit); put(b, 6, (uint64_t)flags);
    if (!quincunx && type != 5)
        for (int k = 1; k <= 4; k++) put(b, 4, (uint64_t)((g * k) & 15));
    put(b, 8, (uint64_t)reserved); put(b, 1, (uint64_t)persistence); put(b, 1, (uint64_t)uar);
}

static size_t finish(struct bits *b)                          /* the alignment bits; returns the payload's bytes */
{
    put(b, 1, 1);
    while (b->n & 7) put(b, 1, 0);
    return b->n / 8;
}

static void check_message(const OhFramePackingSei *r, uint32_t id, int type, int quincunx, int cit, int flags, int g, int reserved,
                          int persistence, int uar)
{
    const int coded = !quincunx && type != 5;
    CHECK(r->present == 1 && r->cancel == 0 && r->id == id, "id %u", r->id);
    CHECK(r->arrangement_type == type && r->quincunx_sampling == quincunx && r->content_interpretation_type == cit, "type %d", r->arrangement_type);
    CHECK(r->spatial_flipping == ((flags >> 5) & 1) && r->frame0_flipped == ((flags >> 4) & 1) && r->field_views == ((flags >> 3) & 1) &&
          r->current_frame_is_frame0 == ((flags >> 2) & 1) && r->frame0_self_contained == ((flags >> 1) & 1) &&
          r->frame1_self_contained == (flags & 1), "flags %d", flags);
    CHECK(r->frame0_grid_position_x == (coded ? (g & 15) : 0) && r->frame0_grid_position_y == (coded ? ((2 * g) & 15) : 0) &&
          r->frame1_grid_position_x == (coded ? ((3 * g) & 15) : 0) && r->frame1_grid_position_y == (coded ? ((4 * g) & 15) : 0), "grid %d", g);
    CHECK(r->reserved_byte == reserved && r->persistence == persistence && r->upsampled_aspect_ratio == uar, "tail");
}

int main(void)
{
    OhFramePackingSei r;
    size_t size;
    int n = 0;

    /* 1. every arrangement type with every flag pattern, quincunx or not */
    for (int type = 0; type < 128; type++)
        for (int flags = 0; flags < 64; flags++) {
            const int quincunx = (type + flags) & 1, cit = (type * 5 + flags) & 63, g = type + flags, reserved = (type * 2 + flags) & 255;
            struct bits b = { 0, 0, 0 };
            message(&b, (uint64_t)(type * 64 + flags), type, quincunx, cit, flags, g, reserved, flags & 1, (flags >> 1) & 1);
            const size_t len = finish(&b);
            uint8_t *u = unit1(b.p, len, &size, 39);
            CHECK(read_copy(u, size, &r) == 1, "type %d flags %d", type, flags);
            check_message(&r, (uint32_t)(type * 64 + flags), type, quincunx, cit, flags, g, reserved, flags & 1, (flags >> 1) & 1);
            free(u); free(b.p); n++;
        }
    printf("%d messages: every type, every flag pattern\n", n);

    /* 2. ids up to 2^32 - 1, one above, and a code of 33 leading zeros; a cancelled message */
    {
        const uint64_t ids[] = { 0, 1, 254, 255, 65535, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu };
        for (size_t k = 0; k < sizeof(ids) / sizeof(ids[0]); k++) {
            struct bits b = { 0, 0, 0 };
            message(&b, ids[k], 4, 0, 2, 0x30, 7, 0, 1, 0);
            const size_t len = finish(&b);
            uint8_t *u = unit1(b.p, len, &size, 39);
            CHECK(read_copy(u, size, &r) == 1 && r.id == (uint32_t)ids[k], "id %llu", (unsigned long long)ids[k]);
            free(u); free(b.p);
        }
        struct bits b = { 0, 0, 0 };
        put_ue(&b, (uint64_t)1 << 32); put(&b, 1, 1); put(&b, 1, 0);
        size_t len = finish(&b);
        uint8_t *u = unit1(b.p, len, &size, 39);
        CHECK(read_copy(u, size, &r) == -1 && all_zero(&r), "an id of 2^32");
        free(u); free(b.p);
        struct bits z = { 0, 0, 0 };
        put(&z, 33, 0); put(&z, 1, 1); put(&z, 34, 0);
        len = finish(&z);
        u = unit1(z.p, len, &size, 39);
        CHECK(read_copy(u, size, &r) == -1 && all_zero(&r), "33 leading zeros");
        free(u); free(z.p);
        struct bits c = { 0, 0, 0 };
        put_ue(&c, 77); put(&c, 1, 1); put(&c, 1, 1);
        len = finish(&c);
        u = unit1(c.p, len, &size, 39);
        CHECK(read_copy(u, size, &r) == 1 && r.cancel == 1 && r.id == 77 && r.upsampled_aspect_ratio == 1 && r.arrangement_type == 0, "cancel");
        CHECK(read_copy(u, size, &r) == 1, "again");
        free(u);
        u = unit1(c.p, len, &size, 40);                        /* a suffix SEI: passed over */
        CHECK(read_copy(u, size, &r) == 0 && all_zero(&r), "suffix");
        free(u); free(c.p);
        printf("ids, refusals, cancel\n");
    }

    /* 3. every truncation of the unit and of the payload; the payload holds runs of zeros, so the unit has emulation-prevention bytes */
    {
        struct bits b = { 0, 0, 0 };
        message(&b, 0, 0, 0, 0, 0, 0, 0, 0, 0);               /* 00 .. 00 behind the first byte */
        const size_t nbits = b.n, len = finish(&b);
        uint8_t *u = unit1(b.p, len, &size, 39);
        CHECK(size > 2 + 2 + len + 1, "emulation prevention bytes were needed");
        CHECK(read_copy(u, size, &r) == 1, "the whole unit");
        check_message(&r, 0, 0, 0, 0, 0, 0, 0, 0, 0);
        for (size_t cut = 0; cut + 1 < size; cut++) {
            const int rc = read_copy(u, cut, &r);
            CHECK((rc == -1 || rc == 0) && all_zero(&r), "unit cut to %zu: %d", cut, rc);
        }
        free(u);
        for (size_t cut = 0; cut <= len; cut++) {
            u = unit1(b.p, cut, &size, 39);
            const int rc = read_copy(u, size, &r), whole = cut * 8 >= nbits;
            CHECK(rc == (whole ? 1 : -1) && (whole || all_zero(&r)), "payload cut to %zu: %d", cut, rc);
            free(u);
        }
        free(b.p);
        printf("truncations\n");
    }

    /* 4. two messages in one unit: the last one counts; a broken second one refuses the unit */
    {
        struct bits a = { 0, 0, 0 }, b = { 0, 0, 0 };
        message(&a, 1, 3, 0, 1, 0x20, 3, 9, 1, 0);
        message(&b, 2, 4, 1, 2, 0x01, 0, 200, 0, 1);
        const size_t la = finish(&a), lb = finish(&b);
        const uint8_t *const p[2] = { a.p, b.p }, *const q[2] = { b.p, a.p };
        const size_t l[2] = { la, lb }, m[2] = { lb, la }, cutl[2] = { la, 2 };
        uint8_t *u = unit(p, l, 2, &size, 39);
        CHECK(read_copy(u, size, &r) == 1, "a, b");
        check_message(&r, 2, 4, 1, 2, 0x01, 0, 200, 0, 1);
        free(u);
        u = unit(q, m, 2, &size, 39);
        CHECK(read_copy(u, size, &r) == 1, "b, a");
        check_message(&r, 1, 3, 0, 1, 0x20, 3, 9, 1, 0);
        free(u);
        u = unit(p, cutl, 2, &size, 39);
        CHECK(read_copy(u, size, &r) == -1 && all_zero(&r), "a, b cut");
        free(u); free(a.p); free(b.p);
        printf("two messages\n");
    }

    /* 5. payloads of every byte value and every length up to 8: accepted or refused, never read past */
    {
        int found = 0, refused = 0;
        for (int v = 0; v < 256; v++)
            for (size_t len = 0; len <= 8; len++) {
                uint8_t p[8];
                for (size_t i = 0; i < len; i++) p[i] = (uint8_t)(v + 37 * (int)i);
                uint8_t *u = unit1(p, len, &size, 39);
                const int rc = read_copy(u, size, &r);
                CHECK(rc == 1 || (rc == -1 && all_zero(&r)), "value %d length %zu: %d", v, len, rc);
                found += rc == 1; refused += rc == -1;
                free(u);
            }
        printf("arbitrary payloads: %d read, %d refused\n", found, refused);
    }

    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("frame packing sei ok\n");
    return 0;
}
