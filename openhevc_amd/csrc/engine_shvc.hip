/*
 * engine_shvc.hip — the engine's SHVC inter-layer reference (host side; kernels in upsample.hip): the up-sampled base-layer
 * picture of upsample_base_layer_frame (hevcdsp_template.c:2164-2438, called at hevc.c:3241), whole or per CTB, and the reference's
 * own CTB path (upblock.h).
 */
#include "engine_impl.h"

/* the window lies inside the enhancement-layer picture and the scales are positive */
static bool up_window_ok(const OhUpsample *u, int w_el, int h_el)
{
    return u->win_left >= 0 && u->win_right >= 0 && u->win_top >= 0 && u->win_bottom >= 0 && u->win_left + u->win_right < w_el &&
           u->win_top + u->win_bottom < h_el && u->scale_x_lum > 0 && u->scale_y_lum > 0 && u->scale_x_cr > 0 && u->scale_y_cr > 0;
}

/* the enhancement layer is smaller than the base layer: no spatial scalability, and the source windows are unbounded */
static bool up_shrinks(const OhUpsample *u) { return u->scale_x_lum > 65536 || u->scale_y_lum > 65536 || u->scale_x_cr > 65536 || u->scale_y_cr > 65536; }

static bool upb_args_ok(const OhUpsample *u, int w_bl, int h_bl, int w_el, int h_el, int log2_ctb)
{
    return u && w_bl > 0 && h_bl > 0 && w_el > 0 && h_el > 0 && log2_ctb >= 4 && log2_ctb <= 6 && up_window_ok(u, w_el, h_el) &&
           u->idx >= OH_UP_DEFAULT && u->idx <= OH_UP_SNR;
}

/* what the tile form and the block form (blocks: also the CTB size and the filter index) check of a call before anything else;
 * *el, *bl: the two pictures.  The tile form gives up the destination's batch (done_seq) as soon as the ids are known. */
static int up_check(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u, bool blocks, int log2_ctb, const char *who, Pic **el_out, Pic **bl_out)
{
    Pic *el = get_pic(e, dst_pic), *bl = get_pic(e, src_pic);
    if (!el || !bl || el == bl)
        FAIL(e, OH_E_ARG, "%s: bad picture ids", who);
    if (!blocks)
        el->done_seq = 0;
    if (el->p.bit_depth != 8 || bl->p.bit_depth != 8 || el->p.chroma_format_idc != 1 || bl->p.chroma_format_idc != 1)
        FAIL(e, OH_E_UNSUPPORTED, "%s: the reference's up-sampler is written for 8-bit 4:2:0 (byte edge buffers, shift 12)", who);
    if (blocks ? !upb_args_ok(u, bl->p.width, bl->p.height, el->p.width, el->p.height, log2_ctb) : !up_window_ok(u, el->p.width, el->p.height))
        FAIL(e, OH_E_ARG, "%s: bad window / scale%s", who, blocks ? " / CTB size" : "");
    if (up_shrinks(u))
        FAIL(e, OH_E_UNSUPPORTED, "%s: the enhancement layer is smaller than the base layer (scale > 1): not a spatial-scalability configuration", who);
    *el_out = el; *bl_out = bl;
    return OH_OK;
}

/* SHVC up-sampling of tiles of the enhancement-layer picture: ctbs == nullptr: the whole picture (the reference's whole-picture
 * slot, hevc.c:3241); else the listed CTBs (raster addresses, CTB size 1 << log2_ctb) — the on-demand granularity of the
 * reference's default build (ff_upsample_block, hevc_filter.c:1370-1426: a CTB is up-sampled when a PU first predicts from it) */
static int upsample_tiles(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u, int log2_ctb, const uint32_t *ctbs, int n_ctbs, const char *who)
{
    if (!e || !u)
        return OH_E_ARG;
    Pic *el, *bl;
    { const int rc = up_check(e, dst_pic, src_pic, u, false, 0, who, &el, &bl); if (rc) return rc; }
    const int w_el = el->p.width, h_el = el->p.height, w_bl = bl->p.width, h_bl = bl->p.height;
    HIPCHK(e, hipSetDevice(e->device));
    const int tile = ctbs ? 1 << log2_ctb : 64;
    const uint32_t *dlist = nullptr;
    OhEngine::Stage *sg = nullptr;
    if (ctbs) {
        if (log2_ctb < 4 || log2_ctb > 6 || n_ctbs < 0)
            FAIL(e, OH_E_ARG, "%s: CTB size / count", who);
        if (!n_ctbs)
            return OH_OK;
        const uint32_t n_ctb = (uint32_t)(((w_el + tile - 1) / tile) * ((h_el + tile - 1) / tile));
        for (int i = 0; i < n_ctbs; i++)
            if (ctbs[i] >= n_ctb)
                FAIL(e, OH_E_ARG, "%s: CTB address %u of %u", who, ctbs[i], n_ctb);
        sg = stage_list(e, ctbs, (size_t)n_ctbs * sizeof(uint32_t));
        if (!sg)
            FAIL(e, OH_E_NOMEM, "%s: no staging buffer", who);
        dlist = (const uint32_t *)sg->p;
    }
    void *const *src = final_planes(bl);
    OhUpPlane a;
    /* luma: BL rows = min(BL height, EL height) (:2220); x clipped to [left, right_end] inclusive (:2223) */
    a.src = src[0]; a.sstride = bl->stride[0]; a.w_bl = w_bl; a.h_bl = h_bl <= h_el ? h_bl : h_el;
    a.dst = el->a[0]; a.dstride = el->stride[0]; a.w_el = w_el; a.h_el = h_el;
    a.left = u->win_left; a.right_end_h = w_el - u->win_right; a.right_end_v = w_el - u->win_right;
    a.top = u->win_top; a.bottom_end = h_el - u->win_bottom;
    a.scale_x = u->scale_x_lum; a.add_x = u->add_x_lum; a.scale_y = u->scale_y_lum; a.add_y = u->add_y_lum; a.y_bias = 0;
    ohk_upsample_plane(&a, 8, tile, tile, dlist, n_ctbs, e->stream);
    /* chroma: BL rows = max(BL height, EL chroma height) >> 1 (:2317-2320); x clipped to [left, right_end - 1] (:2324);
     * the vertical position carries the -4 of :2384.  A CTB's chroma tile has the same index in a grid of half-size tiles. */
    const int wc_el = w_el >> 1, hc_el = h_el >> 1;
    for (int c = 1; c <= 2; c++) {
        a.src = src[c]; a.sstride = bl->stride[c]; a.w_bl = w_bl >> 1; a.h_bl = (h_bl > hc_el ? h_bl : hc_el) >> 1;
        if (a.h_bl > bl->h[c]) a.h_bl = bl->h[c];
        a.dst = el->a[c]; a.dstride = el->stride[c]; a.w_el = wc_el; a.h_el = hc_el;
        a.left = u->win_left >> 1; a.right_end_v = wc_el - (u->win_right >> 1); a.right_end_h = a.right_end_v - 1;
        a.top = u->win_top >> 1; a.bottom_end = hc_el - (u->win_bottom >> 1);
        a.scale_x = u->scale_x_cr; a.add_x = u->add_x_cr; a.scale_y = u->scale_y_cr; a.add_y = u->add_y_cr; a.y_bias = 4;
        ohk_upsample_plane(&a, 4, tile >> 1, tile >> 1, dlist, n_ctbs, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    if (sg) { const int rc = stage_in_use(e, sg, e->stream); if (rc) return rc; }
    el->final_b = false;                                   /* the resampled picture is a finished picture in half 0 */
    return OH_OK;
}

extern "C" int oh_pic_upsample(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u)
{
    return upsample_tiles(e, dst_pic, src_pic, u, 6, nullptr, 0, "oh_pic_upsample");
}

extern "C" int oh_pic_upsample_ctbs(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u, int log2_ctb_size, const uint32_t *ctb_addrs, int n)
{
    if (!ctb_addrs && n)
        return OH_E_ARG;
    /* the reference's block path positions by its block driver and its x2 / x1.5 slots ignore the phase: with scaled reference
     * layer offsets or phase alignment it produces OTHER samples than the whole-picture slot (tests/test_upsample_vs_ref.py
     * records both).  This entry point is the whole-picture arithmetic per CTB, so it stands for the block path only where the
     * reference's two paths agree. */
    if (u && (u->win_left || u->win_right || u->win_top || u->win_bottom))
        FAIL(e, OH_E_UNSUPPORTED, "oh_pic_upsample_ctbs: scaled reference layer offsets — the reference's CTB path and its whole-picture slot differ there; use oh_pic_upsample");
    static const uint32_t none = 0;
    return upsample_tiles(e, dst_pic, src_pic, u, log2_ctb_size, n ? ctb_addrs : &none, n, "oh_pic_upsample_ctbs");
}

/* ---- the reference's CTB path (upblock.h): where its output is defined, and the call ---- */
static void upb_geoms(OhUpBlkGeom g[2], const OhUpsample *u, int w_bl, int h_bl, int w_el, int h_el, int log2_ctb, const OhWindow *conf)
{
    for (int c = 0; c < 2; c++) {
        OhUpBlkGeom &q = g[c];
        q.cr = c; q.idx = u->idx; q.log2_ctb = log2_ctb;
        q.w_el = w_el >> c; q.h_el = h_el >> c;
        q.bl_w = w_bl >> c; q.bl_w_act = w_bl >> c; q.bl_h_act = h_bl >> c;
        q.bl_h = c ? (h_bl > q.h_el ? h_bl : q.h_el) >> 1 : h_bl;          /* hevc_filter.c:1252 */
        q.left = u->win_left >> c; q.right_end = q.w_el - (u->win_right >> c);
        q.top = u->win_top >> c; q.bottom_end = q.h_el - (u->win_bottom >> c);
        q.sx = c ? u->scale_x_cr : u->scale_x_lum; q.ax = c ? u->add_x_cr : u->add_x_lum;
        q.sy = c ? u->scale_y_cr : u->scale_y_lum; q.ay = c ? u->add_y_cr : u->add_y_lum;
        q.dsx = u->scale_x_lum; q.dax = u->add_x_lum; q.dsy = u->scale_y_lum; q.day = u->add_y_lum;
        q.conf_left = conf ? conf->left >> c : 0; q.conf_top = conf ? conf->top >> c : 0;
    }
}

static const char *upb_reason(int r)
{
    switch (r) {
    case UPB_STALE_ROW:    return "its vertical slot reads an intermediate row the window estimate (hevc_filter.c:1260) did not filter: scratch of an earlier call";
    case UPB_BL_ROW:       return "it reads base-layer rows outside the picture";
    case UPB_BL_COL:       return "it reads base-layer columns beyond an edge its call did not emulate";
    case UPB_BL_OVERWRITE: return "its left edge emulation writes over base-layer samples other CTBs read";
    case UPB_FOREIGN_ROW:  return "its chroma rows clip into another CTB's rows";
    }
    return "?";
}

/* the first CTB of the list (all CTBs: ctbs == nullptr) whose output the reference does not define; *reason: UPB_*, *plane: 0 luma 1 chroma */
static int upb_first_bad(const OhUpBlkGeom g[2], int w_el, int h_el, int log2_ctb, const uint32_t *ctbs, int n, int *reason, int *plane)
{
    const int size = 1 << log2_ctb, cw = (w_el + size - 1) >> log2_ctb, nall = cw * ((h_el + size - 1) >> log2_ctb);
    for (int k = 0; k < (ctbs ? n : nall); k++) {
        const int a = ctbs ? (int)ctbs[k] : k, x0 = (a % cw) << log2_ctb, y0 = (a / cw) << log2_ctb;
        for (int c = 0; c < 2; c++) {
            const int r = upb_check(g[c], x0 >> c, y0 >> c);
            if (r) {
                *reason = r; *plane = c;
                return a;
            }
        }
    }
    return -1;
}

extern "C" int oh_upsample_blocks_defined(const OhUpsample *u, int w_bl, int h_bl, int w_el, int h_el, int log2_ctb_size, int *first_bad_ctb)
{
    if (first_bad_ctb)
        *first_bad_ctb = -1;
    if (!upb_args_ok(u, w_bl, h_bl, w_el, h_el, log2_ctb_size))
        return OH_E_ARG;
    if (up_shrinks(u))
        return 0;
    OhUpBlkGeom g[2];
    upb_geoms(g, u, w_bl, h_bl, w_el, h_el, log2_ctb_size, nullptr);
    int reason, plane;
    const int bad = upb_first_bad(g, w_el, h_el, log2_ctb_size, nullptr, 0, &reason, &plane);
    if (first_bad_ctb)
        *first_bad_ctb = bad;
    return bad < 0;
}

extern "C" int oh_pic_upsample_blocks(OhEngine *e, int dst_pic, int src_pic, const OhUpsample *u, int log2_ctb_size,
                                      const OhWindow *el_conf_win, const uint32_t *ctb_addrs, int n)
{
    if (!e || !u || (!ctb_addrs && n) || n < 0)
        return OH_E_ARG;
    Pic *el, *bl;
    { const int rc = up_check(e, dst_pic, src_pic, u, true, log2_ctb_size, "oh_pic_upsample_blocks", &el, &bl); if (rc) return rc; }
    const int w_el = el->p.width, h_el = el->p.height, w_bl = bl->p.width, h_bl = bl->p.height;
    if (el_conf_win && (el_conf_win->left || el_conf_win->right || el_conf_win->top || el_conf_win->bottom))
        FAIL(e, OH_E_UNSUPPORTED, "oh_pic_upsample_blocks: a non-zero enhancement-layer conformance window (the driver positions by it, hevc_filter.c:1196-1197) is not covered yet");
    const int size = 1 << log2_ctb_size, n_all = ((w_el + size - 1) >> log2_ctb_size) * ((h_el + size - 1) >> log2_ctb_size);
    for (int i = 0; ctb_addrs && i < n; i++)
        if (ctb_addrs[i] >= (uint32_t)n_all)
            FAIL(e, OH_E_ARG, "oh_pic_upsample_blocks: CTB address %u of %d", ctb_addrs[i], n_all);
    OhUpBlkArgs a;
    upb_geoms(a.g, u, w_bl, h_bl, w_el, h_el, log2_ctb_size, el_conf_win);
    a.g[1].bl_h_act = bl->h[1] < a.g[1].bl_h_act ? bl->h[1] : a.g[1].bl_h_act;
    int reason = 0, plane = 0;
    const int bad = upb_first_bad(a.g, w_el, h_el, log2_ctb_size, ctb_addrs, n, &reason, &plane);
    if (bad >= 0)
        FAIL(e, OH_E_UNSUPPORTED, "oh_pic_upsample_blocks: the reference's CTB path does not define CTB %d (%s): %s", bad, plane ? "chroma" : "luma",
             upb_reason(reason));
    el->done_seq = 0;
    const int cnt = ctb_addrs ? n : n_all;
    if (!cnt)
        return OH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    const uint32_t *dlist = nullptr;
    OhEngine::Stage *sg = nullptr;
    if (ctb_addrs) {
        sg = stage_list(e, ctb_addrs, (size_t)n * sizeof(uint32_t));
        if (!sg)
            FAIL(e, OH_E_NOMEM, "oh_pic_upsample_blocks: no staging buffer");
        dlist = (const uint32_t *)sg->p;
    }
    void *const *src = final_planes(bl), *const *dst = final_planes(el);   /* CTBs not listed keep their samples */
    for (int c = 0; c < 3; c++) {
        a.src[c] = src[c]; a.sstride[c] = (int32_t)bl->stride[c];
        a.dst[c] = dst[c]; a.dstride[c] = (int32_t)el->stride[c];
    }
    a.ctbs_x = (w_el + size - 1) >> log2_ctb_size;
    ohk_upsample_blocks(&a, dlist, cnt, e->stream);
    HIPCHK(e, hipGetLastError());
    if (sg) { const int rc = stage_in_use(e, sg, e->stream); if (rc) return rc; }
    return OH_OK;
}
