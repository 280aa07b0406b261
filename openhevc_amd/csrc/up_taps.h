/*
 * up_taps.h — the 16-phase SHVC up-sampling taps (the reference's up_sample_filter_luma / up_sample_filter_chroma, hevcdsp.c:948-986):
 * row p holds the taps of phase p / 16 of a sample spacing, 8 for luma with the centre at tap 3, 4 for chroma with the centre at tap 1;
 * every row sums to 64.  The one place the numbers are written down: upsample.hip's whole-picture slot, upblock.h's CTB path (which
 * appends the rows of the reference's x2 / x1.5 variants) and packing_common.h's frame-packing up-sampler initialise their tables from
 * these lists.
 */
#ifndef OHEVC_UP_TAPS_H
#define OHEVC_UP_TAPS_H

#define UP_TAPS_LUMA_ROWS \
    { 0, 0, 0, 64, 0, 0, 0, 0 }, { 0, 1, -3, 63, 4, -2, 1, 0 }, { -1, 2, -5, 62, 8, -3, 1, 0 }, { -1, 3, -8, 60, 13, -4, 1, 0 }, \
    { -1, 4, -10, 58, 17, -5, 1, 0 }, { -1, 4, -11, 52, 26, -8, 3, -1 }, { -1, 3, -9, 47, 31, -10, 4, -1 }, { -1, 4, -11, 45, 34, -10, 4, -1 }, \
    { -1, 4, -11, 40, 40, -11, 4, -1 }, { -1, 4, -10, 34, 45, -11, 4, -1 }, { -1, 4, -10, 31, 47, -9, 3, -1 }, { -1, 3, -8, 26, 52, -11, 4, -1 }, \
    { 0, 1, -5, 17, 58, -10, 4, -1 }, { 0, 1, -4, 13, 60, -8, 3, -1 }, { 0, 1, -3, 8, 62, -5, 2, -1 }, { 0, 1, -2, 4, 63, -3, 1, 0 }

#define UP_TAPS_CHROMA_ROWS \
    { 0, 64, 0, 0 }, { -2, 62, 4, 0 }, { -2, 58, 10, -2 }, { -4, 56, 14, -2 }, { -4, 54, 16, -2 }, { -6, 52, 20, -2 }, { -6, 46, 28, -4 }, { -4, 42, 30, -4 }, \
    { -4, 36, 36, -4 }, { -4, 30, 42, -4 }, { -4, 28, 46, -6 }, { -2, 20, 52, -6 }, { -2, 16, 54, -4 }, { -2, 14, 56, -4 }, { -2, 10, 58, -2 }, { 0, 4, 62, -2 }

#endif
