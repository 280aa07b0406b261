/* kernels.h — the launchers of the kernel files and what they take (internal to libohevc_hip.so): the argument blocks of the picture
 * services, one per .hip file and passed by value in the kernel arguments, with the tile sizes that the host shares, then the launchers
 * of the services and of the decode passes (mc / residual / intra / deblock / sao / upsample / prep / bs .hip).  Array sizes are the
 * public constants of include/ohevc_hip.h. */
#ifndef OHEVC_KERNELS_H
#define OHEVC_KERNELS_H

#include <hip/hip_runtime.h>
#include "../../include/ohevc_hip.h"
#include "dev_frame.h"
#include "upblock.h"
#include "packing_common.h"

/* the reference's CTB up-sampling path (upsample.hip: upsample_block_kernel): planes and their geometry (g[0] luma, g[1] chroma) */
struct OhUpBlkArgs {
    OhUpBlkGeom g[2];
    const void *src[3]; void *dst[3];
    int32_t sstride[3], dstride[3];
    int32_t ctbs_x;
};

/* one plane to hash: its packed rows (one MD5 chain, md5.hip; CRC / checksum tasks, hash.hip) */
struct OhMd5Job {
    const void *base;            /* first sample of the plane */
    uint32_t    pitch;           /* bytes between rows */
    uint32_t    row_bytes;       /* bytes hashed per row */
    uint32_t    rows;
    uint32_t    bps;             /* bytes per sample (1, 2): the checksum's sample column; MD5 does not read it */
};
enum { OH_HASH_TASK = 128 << 10 };   /* packed plane bytes per CRC / checksum workgroup (hash.hip) */

/* picture conversion (convert.hip): what one launch needs, passed by value in the kernel arguments (no job table in memory that a
 * later call could overwrite before the launch runs).  Every picture of a launch has the same geometry; src: its finished planes. */
struct OhConvArgs {
    const void *src[OH_CONV_MAX_PICS][3]; /* pictures x planes */
    void       *dst;             /* image of the launch's first picture */
    uint64_t    image_stride;    /* bytes from one image to the next */
    int32_t     pitch[3];        /* bytes between rows of each plane */
    int32_t     cw, ch;          /* coded chroma plane size (clamping of the linear filter) */
    int32_t     left, top, W, H; /* window, luma samples */
    int32_t     cf, bd;          /* chroma_format_idc, bit depth */
    int32_t     filter;          /* 0 nearest, 1 linear */
    int32_t     nc;              /* interleaved RGB: 3 or 4 channels */
    int32_t     k[9];            /* oh_convert_coeffs: cy, crv, cgu, cgv, cbu, yoff, mid, S, D */
};

/* picture import (import.hip): the inverse of OhConvArgs.  dst: half 0 of the destination pictures, src: the image of the
 * launch's first picture in caller-owned device memory; every picture of a launch has the same geometry. */
struct OhImpArgs {
    void       *dst[OH_CONV_MAX_PICS][3]; /* pictures x planes */
    const void *src;             /* image of the launch's first picture */
    uint64_t    image_stride;    /* bytes from one image to the next */
    int32_t     pitch[3];        /* bytes between rows of each plane */
    int32_t     pw[2], ph[2];    /* coded plane size: luma, chroma */
    int32_t     left, top, W, H; /* window, luma samples */
    int32_t     cf, bd;          /* chroma_format_idc, bit depth */
    int32_t     filter;          /* RGB images, 4:2:0 / 4:2:2: 0 point, 1 linear */
    int32_t     nc;              /* interleaved RGB: 3 or 4 channels */
    int32_t     k[13];           /* oh_import_coeffs: ry gy by ru gu bu rv gv bv yoff mid S D */
};

/* colour conversion (colour.hip): the geometry and the matrix of an RGB conversion (k: the coefficients for 16 bit), the
 * integers of oh_colour_tables' misc, and the three tables in device memory that the engine owns and fills on the stream in front of the
 * launches: A at int32 0, G at OH_COLT_G, B at OH_COLT_B, OH_COLT_N in all (each table padded to whole 16-byte granules). */
enum { OH_COLT_G = 4100, OH_COLT_B = 4100 + 1604, OH_COLT_N = 4100 + 2 * 1604,
       OH_COL_ROWS = 8 };            /* image rows per workgroup: it loads the tables once for all of them */
struct OhColArgs {
    OhConvArgs     c;
    const int32_t *tab;
    int32_t        misc[OH_COL_NMISC];
};

/* light-level statistics (light.hip): the geometry and the 16-bit matrix of an RGB conversion (c.dst, c.image_stride and
 * c.nc are not read), table A of oh_colour_tables in device memory (OH_COLT_G int32: padded to whole 16-byte granules) and the result
 * of the launch's first picture, both in device memory that the engine owns and prepares on the stream in front of the launch. */
enum { OH_LL_ROWS = 32,              /* image rows per workgroup: it loads the table once for all of them */
       OH_LL_CW = 1024 };            /* image columns per workgroup */
struct OhLightDev {                  /* one picture's sums; cleared to zero in front of the launch */
    unsigned long long sum;
    uint32_t max, not_min;           /* not_min: the largest ~v, so that zero is the neutral start of all four */
    uint32_t hist[OH_LL_NBINS];
};
struct OhLightArgs {
    OhConvArgs     c;
    const int32_t *tab;
    OhLightDev    *res;
    int32_t        w[3];             /* Q14 luminance weights (misc[9..11] of oh_colour_tables) */
    int32_t        luma;             /* 1: OH_NORM_LUMA, 0: OH_NORM_MAXRGB */
};

/* picture comparison (compare.hip): the finished planes of the pairs of one launch by value in the kernel arguments, two
 * plane classes (0 luma, 1 chroma) with the plane's window and its tiling, and the results of the launch's first pair in device memory
 * that the engine owns and clears on the stream in front of the launch. */
enum { OH_CMP_TW = 256,              /* plane columns per workgroup tile: 64 blocks of 4 x 4 */
       OH_CMP_TH = 32,               /* plane rows per workgroup tile: 8 block rows */
       OH_CMP_SLOTS = 8 };           /* partial results per plane of a pair: tile t adds into slot t % OH_CMP_SLOTS, the host combines them */
struct OhCmpDev {                    /* one slot of one plane of one pair, a 64-byte line of its own; cleared to zero in front of the launch */
    unsigned long long differing, sad, sse;
    unsigned long long ssim_sum;     /* two's complement of the signed sum */
    uint32_t max_abs, not_first;     /* not_first: the largest ~(y * w + x) of a differing sample, so that zero is the neutral start */
    uint32_t pad[6];
};
struct OhCmpClass {
    int32_t x0, y0, w, h;            /* the plane's window: origin in the plane, size */
    int32_t tx, ty;                  /* tiles across and down: at least one each */
};
struct OhCmpArgs {
    const void *a[OH_CONV_MAX_PICS][3], *b[OH_CONV_MAX_PICS][3]; /* pairs x planes: the finished halves */
    OhCmpDev   *res;                 /* [pair][3][OH_CMP_SLOTS] */
    OhCmpClass  k[2];
    int32_t     pitch[3];            /* bytes between rows of each plane */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
    int32_t     ssim;                /* 1: OH_CMP_SSIM */
};

/* picture composition (compose.hip): the finished halves of the destinations of one launch set by value in the kernel
 * arguments, two plane classes (0 luma, 1 chroma) with the area the call touches and its tiling, and the layers in device memory that
 * the engine owns and fills on the stream in front of the launches: the layers that are not wholly outside, in list order, with their
 * geometry in both classes, then per layer and destination of the launch set the source's finished planes and the alpha plane. */
enum { OH_CPS_TW = 64,               /* 16-byte granules of a destination row per workgroup tile: a wave takes one row of them */
       OH_CPS_TH = 4 };              /* rows per tile */
struct OhCpsLayer {                  /* [class] where a member has two entries */
    int32_t x0[2], y0[2], x1[2], y1[2];  /* the rectangle clipped to the destination plane, plane samples: [x0, x1) x [y0, y1) */
    int32_t ox[2], oy[2];            /* source sample = destination sample + (ox, oy) */
    int32_t dx[2], dy[2];            /* where the unclipped rectangle starts in the destination plane: the origin of the alpha plane */
    int32_t spitch[2];               /* bytes between rows of the source's planes */
    int32_t opacity;                 /* 0 .. 256 */
    int32_t has_alpha;
    int64_t a_ps, a_rs;              /* bytes from one luma alpha to the next, from one row of them to the next */
};
struct OhCpsSrc {
    const void    *p[3];             /* the source's finished planes */
    const uint8_t *alpha;            /* the alpha of this destination's rectangle sample (0, 0); not read without has_alpha */
};
struct OhCpsClass {
    int32_t gx0, gx1, y0, y1;        /* the touched area: granules [gx0, gx1) of rows [y0, y1) */
    int32_t tx, ty;                  /* tiles across and down */
};
struct OhCpsArgs {
    void             *dst[OH_CONV_MAX_PICS][3]; /* destinations x planes: the finished halves */
    const OhCpsLayer *layers;        /* [n_layers] */
    const OhCpsSrc   *srcs;          /* [n_layers][n_pics] */
    OhCpsClass        k[2];
    int32_t           pitch[3];      /* bytes between rows of each destination plane */
    int32_t           np, bd, cf;    /* planes: 1 or 3; bit depth; chroma_format_idc */
    int32_t           n_layers, n_pics;
    int32_t           fill;          /* 1: every sample starts as fill_v[plane] and the destination is not read */
    int32_t           fill_v[3];
};

/* picture reformatting (reformat.hip): the finished planes of the sources and half 0 of the destinations of one launch
 * by value in the kernel arguments; every picture of a launch has the same geometry.  Two plane classes (0 luma, 1 chroma). */
enum { OH_RF_SEG = 4096 };           /* plane samples per workgroup segment: of the destination row, or of the source row where chroma is
                                        sub-sampled horizontally on the way (then OH_RF_SEG / 2 destination samples) */
struct OhRfArgs {
    const void *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void       *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    int32_t     spitch[3], dpitch[3];/* bytes between rows of each plane */
    int32_t     sw[2], sh[2];        /* coded size of the source planes (sw[1] = 0: 4:0:0) */
    int32_t     dw[2], dh[2];        /* coded size of the destination planes (dw[1] = 0: 4:0:0) */
    int32_t     scf, dcf;            /* chroma_format_idc of sources and destinations */
    int32_t     sbd, dbd;            /* bit depths */
    int32_t     depth, down, up;     /* OhReformat */
};

/* picture orientation (orient.hip): the finished planes of the sources and half 0 of the destinations of one launch by
 * value in the kernel arguments; every picture of a launch has the same geometry.  Two plane classes (0 luma, 1 chroma). */
enum { OH_OR_TILE = 64,              /* edge of the square tile of destination samples that one workgroup of the transposing kernel makes */
       OH_OR_SEG = 4096 };           /* destination samples of one row per workgroup of the row kernel (orientations 0 .. 3) */
struct OhOrArgs {
    const void *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void       *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    int32_t     spitch[3], dpitch[3];/* bytes between rows of each plane */
    int32_t     x0[2], y0[2];        /* origin of the plane's window S in the source plane */
    int32_t     ws[2], hs[2];        /* size of S, plane samples */
    int32_t     dw[2], dh[2];        /* coded size of the destination planes */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
    int32_t     orientation;         /* OH_ORIENT_* bits */
};

/* picture warping (warp.hip): the finished planes of the sources and half 0 of the destinations of one launch by value
 * in the kernel arguments; every picture of a launch has the same geometry.  Two plane classes (0 luma, 1 chroma).  The tile of one
 * workgroup and its LDS budget are WARP_TW, WARP_TH and WARP_LDS of warp_common.h, which the host's oh_warp_paths shares. */
struct OhWarpArgs {
    const void *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void       *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    int64_t     m[9];                /* OhWarp.m */
    int32_t     spitch[3], dpitch[3];/* bytes between rows of each plane */
    int32_t     x0[2], y0[2];        /* origin of the plane's window in the source plane */
    int32_t     ws[2], hs[2];        /* size of the plane's window */
    int32_t     iw[2], ih[2];        /* size of the image in the destination planes */
    int32_t     dw[2], dh[2];        /* coded size of the destination planes */
    int32_t     sx, sy;              /* oh_hshift / oh_vshift of the chroma planes */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
    int32_t     mode, filter, border;/* OhWarp */
    int32_t     fill[3];
};

/* fields and deinterlacing (deinterlace.hip): the planes of the pictures of one launch by value in the kernel arguments;
 * every frame of a launch has one geometry, every field another.  Two plane classes (0 luma, 1 chroma).  What the four pictures of
 * index i are depends on the call:
 *   ohk_deinterlace          pic[0] prev, pic[1] cur, pic[2] next (finished halves; prev and next are read by OH_DEINT_ADAPTIVE only),
 *                            pic[3] half 0 of the destination;
 *   ohk_fields, weave        pic[0] top field, pic[1] bottom field (finished halves), pic[3] half 0 of the frame;
 *   ohk_fields, separate     pic[0] the frame (finished half), pic[2] / pic[3] half 0 of the top / bottom field (sides: which are made). */
enum { OH_DI_SEG = 4096 };           /* destination samples of one row per workgroup */
enum { OH_DI_WEAVE = 0, OH_DI_SEPARATE };
struct OhDiArgs {
    void       *pic[4][OH_CONV_MAX_PICS][3]; /* role x pictures x planes */
    int32_t     pitch[3];            /* bytes between rows of each plane: of the frames (ohk_fields), of every picture (ohk_deinterlace) */
    int32_t     fpitch[3];           /* ohk_fields: bytes between rows of each plane of the fields */
    int32_t     w[2], h[2];          /* coded size of the planes: of the frames (ohk_fields), of every picture (ohk_deinterlace) */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
    int32_t     op, sides;           /* ohk_fields: OH_DI_WEAVE / OH_DI_SEPARATE; separate: bit 0 top, bit 1 bottom */
    int32_t     mode, parity, kept_first;    /* ohk_deinterlace: OhDeinterlace */
};

/* picture filters (filter.hip): the planes of the pictures of one launch by value in the kernel arguments, and the taps
 * with them; every picture of a launch has the same geometry.  Two plane classes (0 luma, 1 chroma). */
enum { OH_FLT_TW = 128,              /* destination samples across one workgroup's tile: the horizontal unit */
       OH_FLT_TH = 32 };             /* destination rows of a tile: the vertical unit */
struct OhFilterArgs {
    const void *src[3][OH_CONV_MAX_PICS][3]; /* prev, src, next (finished halves; prev and next are read by OH_FILTER_TEMPORAL only) x
                                        pictures x planes */
    void       *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    int32_t     pitch[3];            /* bytes between rows of each plane */
    int32_t     w[2], h[2];          /* coded size of the planes */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
    int32_t     mode, planes;        /* OhFilter */
    int32_t     radius;              /* CONVOLVE, UNSHARP: the largest nh / 2, nv / 2 of both classes */
    int32_t     taps_h[2][15], taps_v[2][15];   /* the taps of each class, centred: entry OH_FILTER_MAX_TAPS / 2 is the middle tap, zeros around */
    int32_t     amount[2], threshold[2];
};

/* histograms of the code values (histogram.hip): the finished planes of the pictures of one launch by value in the kernel
 * arguments, two plane classes (0 luma, 1 chroma) with the plane's window and the 16-byte granules of a row that cover it, and the bins
 * of the launch's first picture in device memory that the engine owns and clears on the stream in front of the launch. */
enum { OH_HG_ROWS = 8,               /* window rows per workgroup: all the granules of each */
       OH_HG_BINS = OH_HIST_BINS };  /* uint32 per plane of a picture in res */
struct OhHistClass {
    int32_t x0, y0, w, h;            /* the plane's window: origin in the plane, size */
    int32_t g0, ng;                  /* the first granule of a plane row that holds a sample of the window, and how many do */
    int32_t tiles;                   /* workgroups per plane: ceil(h / OH_HG_ROWS) */
};
struct OhHistArgs {
    const void *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    uint32_t   *res;                 /* [picture][3][OH_HG_BINS] */
    OhHistClass k[2];
    int32_t     pitch[3];            /* bytes between rows of each plane */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
};

/* look-up tables (lut.hip): the finished planes of the sources and half 0 of the destinations of one launch by value in
 * the kernel arguments; every picture of a launch has the same geometry.  Two plane classes (0 luma, 1 chroma).  tab: three tables of
 * OH_LUT_MAX uint16 each in device memory that the engine owns and fills on the stream in front of the launch. */
enum { OH_LUT_ROWS = 16,             /* plane rows per workgroup: it loads its plane's table once for all of them */
       OH_LUT_UNIT = 16,             /* samples a lane takes at a time: whole 16-byte granules of either sample type */
       OH_LUT_MAX = 4096 };          /* entries of a table at 12 bit */
struct OhLutArgs {
    const void     *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void           *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    const uint16_t *tab;             /* [3][OH_LUT_MAX] */
    int32_t         spitch[3], dpitch[3];   /* bytes between rows of each plane */
    int32_t         w[2], h[2];      /* coded size of the planes */
    int32_t         np, sbd, dbd;    /* planes: 1 or 3; bit depths */
    int32_t         planes;          /* bit c set: plane c goes through its table; clear: it is copied (sbd == dbd) */
};

/* film grain (grain.hip): the finished planes of the sources and half 0 of the destinations of one launch by value in
 * the kernel arguments; every picture of a launch has the same geometry.  Two plane classes (0 luma, 1 chroma).  tab, seeds and patterns
 * lie in device memory that the engine owns: the tables and seeds of the call, filled on the stream in front of the launches, and the
 * 169 patterns, filled once. */
struct OhGrainArgs {
    const void     *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void           *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    const uint32_t *tab;             /* [3][OH_GRAIN_ENTRIES] */
    const uint32_t *seeds;           /* of the launch's first picture on */
    const int8_t   *patterns;        /* [13][13][32][32]: grain_pattern_index of grain_common.h */
    int32_t         pitch[3];        /* bytes between rows of each plane */
    int32_t         w[2], h[2];      /* coded size of the planes */
    int32_t         tx[2], ty[2];    /* workgroups across (GRAIN_TW blocks each) and down (a row of blocks each) a plane */
    int32_t         np, bd;          /* planes: 1 or 3; bit depth */
    int32_t         planes, blending, log2_scale;   /* OhGrain */
};

/* colour remapping (remap.hip): the finished planes of the sources and half 0 of the destinations of one launch by value
 * in the kernel arguments; every picture is 4:4:4, the sources alike and the destinations alike.  The six tables (pre 0 .. 2, post
 * 0 .. 2) are OH_LUT_MAX uint16 each in device memory that the engine owns and fills on the stream in front of the launch. */
enum { OH_REMAP_ROWS = 8 };          /* picture rows per workgroup: it loads the six tables once for all of them.  Coded heights are
                                      * multiples of the minimum coding block of 8, so no band is ever cut; measured against 4, 16, 32, 64 */
struct OhRemapArgs {
    const void     *src[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void           *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    const uint16_t *tab;             /* [6][OH_LUT_MAX] */
    int32_t         spitch[3], dpitch[3];   /* bytes between rows of each plane */
    int32_t         w, h;            /* coded size of every plane */
    int32_t         sbd, dbd;        /* bit depth of sources and destinations */
    int32_t         coeff[9], log2_denom;   /* OhRemap: the matrix, row-major */
    int32_t         identity;        /* the matrix leaves the pre-table values as they are */
    int32_t         rows;            /* picture rows per workgroup */
};

/* frame packing (packing.hip): the planes of the packed pictures and of the two views of one launch by value in the kernel
 * arguments; every packed picture of a launch has one geometry, every view another.  Two plane classes (0 luma, 1 chroma).
 *   ohk_unpack   packed: the finished halves; view[v]: half 0 of the views that `views` names (bit v)
 *   ohk_pack     view[0], view[1]: the finished halves; packed: half 0 of the destinations */
enum { OH_PK_SEG_BYTES = 4096 };     /* bytes of one destination row per workgroup: a 16-byte granule per lane */
struct OhPkArgs {
    void       *packed[OH_PK_MAX_PICS][3];  /* pictures x planes: 32 packed pictures and their 64 views keep the arguments below 4 KiB */
    void       *view[2][OH_PK_MAX_PICS][3]; /* view x pictures x planes */
    int32_t     ppitch[3], vpitch[3];/* bytes between rows of each plane: packed pictures, views */
    int32_t     dw[2], dh[2];        /* coded size of the destination planes: the views (ohk_unpack), the packed pictures (ohk_pack) */
    PkPlane     pl[2];               /* packing_common.h: the geometry of each plane class */
    int32_t     flip[2], g[2];       /* per view: stored mirrored; the grid position on the packed axis */
    int32_t     np, bd;              /* planes: 1 or 3; bit depth */
    int32_t     views;               /* ohk_unpack: bit v: view v is made */
};

/* motion search and compensation (motion.hip): the finished planes of the pictures of one launch by value in the kernel
 * arguments; every picture of a launch has the same geometry.  The centres, the field and the results of the launch's first picture lie
 * in device memory that the engine owns and fills or clears on the stream in front of the launch. */
enum { OH_MO_REACH = 4 };            /* reference samples beyond the integer range on either side that the sub-sample stages may read:
                                        three quarters further, and the 8-tap filter's three before and four behind */
struct OhMoVec { int16_t x, y; };    /* a vector (quarter samples) of a field, or a centre (integer samples) */
struct OhMoDev { int16_t x, y; uint32_t sad, sad_centre; };  /* OhMotionVector */
struct OhMoSearchArgs {
    const void    *cur[OH_CONV_MAX_PICS], *ref[OH_CONV_MAX_PICS]; /* pairs: the finished luma planes */
    const OhMoVec *centres;          /* [pair][bh][bw], or null: all zero */
    OhMoDev       *res;              /* [pair][bh][bw] */
    int32_t        pitch;            /* bytes between luma rows */
    int32_t        w, h, bd;         /* coded luma size, bit depth */
    int32_t        block, bw, bh;    /* 8 or 16; blocks across and down */
    int32_t        rx, ry, subpel, lambda;
};
struct OhMoCompArgs {
    const void    *ref[OH_CONV_MAX_PICS][3]; /* pictures x planes: the finished halves */
    void          *dst[OH_CONV_MAX_PICS][3]; /* half 0 of the destinations */
    const OhMoVec *field;            /* [picture][bh][bw] */
    int32_t        pitch[3];         /* bytes between rows of each plane */
    int32_t        w[2], h[2];       /* coded size of the planes */
    int32_t        hs, vs;           /* oh_hshift / oh_vshift of the chroma planes */
    int32_t        np, bd;           /* planes: 1 or 3; bit depth */
    int32_t        block, bw, bh;
};

/* picture resizing (resize.hip): what one launch set needs, by value in the kernel arguments like OhConvArgs.  Two plane
 * classes (0 luma, 1 chroma), each with its own geometry and tap tables; the tables live in device memory that the engine owns and
 * fills (engine_pics.hip: oh_pics_resize, from pics_math.hip: oh_resize_taps) on the stream in front of the launches. */
enum { OH_RESIZE_VROWS = 8,          /* image rows per workgroup of the vertical pass */
       OH_RESIZE_LDS = 32 << 10,     /* bytes of staged source rows per workgroup of the horizontal pass */
       OH_RESIZE_SPAN = 4096,        /* most source samples of one staged row */
       OH_RESIZE_HROWS = 16 };       /* most source rows per workgroup of the horizontal pass */
struct OhResizeClass {
    int32_t  x0, y0;                 /* window origin in the plane */
    int32_t  sh;                     /* window rows */
    int32_t  tw, th;                 /* image size in the plane */
    int32_t  cw, ch;                 /* coded size of the destination plane */
    int32_t  src_pitch, dst_pitch;   /* bytes between rows */
    int32_t  mid_stride;             /* int16 between rows of the intermediate (even) */
    int32_t  segw, rpw, row_bytes;   /* horizontal pass: image columns and source rows per workgroup, LDS bytes per staged row */
    int32_t  h_stride;               /* columns between the quad rows of h_k */
    int32_t  h_groups, v_groups;     /* workgroup rows of the two passes for one plane of this class */
    const int32_t *h_first, *h_cnt;  /* per image column: first source column inside the window, taps */
    const int32_t *h_f4, *h_n4;      /* the same as quads of source columns: h_first moved down to a multiple of four plane columns, quads */
    const int16_t *h_k;              /* [quad][h_stride][4]: coefficients of each image column, zero in front of its first and behind its last tap */
    const int32_t *v_first, *v_cnt, *v_off;  /* per group of OH_RESIZE_VROWS image rows: first intermediate row, row PAIRS, offset into v_k */
    const int32_t *v_k;              /* [pair][OH_RESIZE_VROWS]: (coefficient of the even row, of the odd row) of each image row, zero where a row has no tap */
};
struct OhResizeArgs {
    const void *src[OH_RESIZE_MAX_PICS][3]; /* pictures x planes: the finished half */
    void       *dst[OH_RESIZE_MAX_PICS][3]; /* the half the image is written to */
    int16_t    *mid;                 /* intermediate of the launch set's first picture */
    uint64_t    mid_pic;             /* int16 from one picture's intermediate to the next */
    uint64_t    mid_plane[3];        /* int16 from there to each plane's */
    OhResizeClass k[2];
    int32_t     np;                  /* planes: 1 or 3 */
    int32_t     bd;
};

extern "C" {
int  ohk_init(void);
/* n pictures of a: horizontal pass into a.mid, vertical pass into the destinations, then the replicated padding where pad is set */
void ohk_resize(const OhResizeArgs *a, int n, int pad, hipStream_t st);
void ohk_md5(const OhMd5Job *jobs, int n, void *digests, hipStream_t st);
/* format / sample: OH_CONV_* (checked by the caller); n pictures of a.src */
void ohk_convert(const OhConvArgs *a, int format, int sample, int n, hipStream_t st);
/* format / sample: OH_CONV_* of the images (checked by the caller); n pictures of a.dst */
void ohk_import(const OhImpArgs *a, int format, int sample, int n, hipStream_t st);
/* format: an RGB format, sample: U8 .. F32 (checked by the caller); n pictures of a.c.src */
void ohk_colour(const OhColArgs *a, int format, int sample, int n, hipStream_t st);
/* n pictures of a.c.src into a.res[0 .. n) */
void ohk_light(const OhLightArgs *a, int n, hipStream_t st);
/* n pairs of a.a / a.b into a.res[0 .. 3 n OH_CMP_SLOTS) */
void ohk_compare(const OhCmpArgs *a, int n, hipStream_t st);
/* n destinations of a.dst, composed in place: a.layers over what they hold, or over a.fill_v */
void ohk_compose(const OhCpsArgs *a, int n, hipStream_t st);
/* n sources of a.src into the n destinations of a.dst */
void ohk_reformat(const OhRfArgs *a, int n, hipStream_t st);
/* n sources of a.src, oriented, into the n destinations of a.dst */
void ohk_orient(const OhOrArgs *a, int n, hipStream_t st);
/* n sources of a.src, warped, into the n destinations of a.dst */
void ohk_warp(const OhWarpArgs *a, int n, hipStream_t st);
/* n pictures of a.pic[1] (with a.pic[0] and a.pic[2] around them in time) deinterlaced into the n destinations of a.pic[3] */
void ohk_deinterlace(const OhDiArgs *a, int n, hipStream_t st);
/* n pairs of fields woven into n frames, or n frames separated into one or two fields each */
void ohk_fields(const OhDiArgs *a, int n, hipStream_t st);
/* n pictures of a.src[1] (with a.src[0] and a.src[2] around them in time) filtered into the n destinations of a.dst */
void ohk_filter(const OhFilterArgs *a, int n, hipStream_t st);
/* the bins of n pictures of a.src into a.res[0 .. 3 n OH_HG_BINS) */
void ohk_histogram(const OhHistArgs *a, int n, hipStream_t st);
/* n sources of a.src through a.tab into the n destinations of a.dst */
void ohk_lut(const OhLutArgs *a, int n, hipStream_t st);
/* n sources of a.src with grain added into the n destinations of a.dst */
void ohk_grain(const OhGrainArgs *a, int n, hipStream_t st);
/* n sources of a.src remapped into the n destinations of a.dst */
void ohk_remap(const OhRemapArgs *a, int n, hipStream_t st);
/* n packed pictures of a.packed unpacked into the views of a.view that a.views names */
void ohk_unpack(const OhPkArgs *a, int n, hipStream_t st);
/* n pairs of views of a.view packed into the n pictures of a.packed */
void ohk_pack(const OhPkArgs *a, int n, hipStream_t st);
/* the blocks of n pairs of a.cur / a.ref searched into a.res[0 .. n bw bh) */
void ohk_motion_search(const OhMoSearchArgs *a, int n, hipStream_t st);
/* n pictures of a.ref compensated by a.field[0 .. n bw bh) into the n destinations of a.dst */
void ohk_motion_compensate(const OhMoCompArgs *a, int n, hipStream_t st);
void ohk_hash(int kind,const OhMd5Job *jobs, const uint32_t *first, const uint32_t *task_map, int n_jobs, int n_tasks, uint32_t *partials,
              uint32_t *out, hipStream_t st);
void ohk_inter(const OhBatch *B, int n, const OhPicParams *p, uint32_t max_luma, uint32_t max_chroma, hipStream_t st);
void ohk_residual(const OhBatch *B, int n, const OhPicParams *p, const uint32_t max_cnt[4], hipStream_t st);
void ohk_cross(const OhBatch *B, int n, const OhPicParams *p, uint32_t max_cross, hipStream_t st);
void ohk_intra_dag_reset(const OhBatch *B, int n, uint32_t max_ictu, uint32_t *tickets, hipStream_t st);
void ohk_intra_dag(const OhBatch *B, int n, const OhPicParams *p, const OhIntraLaunch *l, uint32_t max_ictu, uint32_t *ticket,
                   uint32_t spin_limit, hipStream_t st);
void ohk_intra_direct(const OhBatch *B, int n, const OhPicParams *p, uint32_t max_ictu, uint32_t *ticket, uint32_t spin_limit, hipStream_t st);
void ohk_deblock(const OhBatch *B, int n, const OhPicParams *p, int horiz, hipStream_t st);
void ohk_upsample_plane(const OhUpPlane *a, int taps, int tw, int th, const uint32_t *list, int n_list, hipStream_t st);
void ohk_upsample_blocks(const OhUpBlkArgs *a, const uint32_t *list, int n, hipStream_t st);
void ohk_sao(const OhBatch *B, int n, const OhPicParams *p, hipStream_t st);
/* one array of a page-locked work list: where it lies on the host, where it goes in the arena */
struct OhPullSeg { const void *src; void *dst; uint64_t bytes; };
void ohk_pull(const OhPullSeg *segs, int nseg, size_t total_bytes, hipStream_t st);
void ohk_prepare(const OhBatch *B, int nb, const OhPrepCounts *max_counts, uint32_t max_mc_runs, uint32_t max_cross, hipStream_t st);
void ohk_bs_derive(const OhPicParams *p, const void *mvf, const void *cbf, const void *call_log2, const void *ctb_flags,
                   int across_tiles, void *vbs, void *hbs, hipStream_t st);
}
#endif
