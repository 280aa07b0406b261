/* pics_math.h — what engine_pics.hip uses of the host arithmetic in pics_math.hip beside the library's own entry points
 * (include/ohevc_hip.h: oh_convert_coeffs, oh_resize_taps, ...).  Internal. */
#ifndef OHEVC_PICS_MATH_H
#define OHEVC_PICS_MATH_H

#include <string>
#include <vector>
#include "../../include/ohevc_hip.h"

#ifndef OH_INTERNAL
#define OH_INTERNAL __attribute__((visibility("hidden")))    /* shared between the library's files, not part of its ABI */
#endif

OH_INTERNAL void window_size(const OhPicParams *p, const OhWindow &w, int *W, int *H);
OH_INTERNAL void class_window(const OhPicParams *p, const OhWindow &w, int q, int32_t *x0, int32_t *y0, int32_t *ws, int32_t *hs);
OH_INTERNAL bool crop_window_ok(const OhPicParams *p, const OhWindow &w, bool aligned, std::string *why);
OH_INTERNAL int ids_apart(const int *dst_ids, int nd, const int *src_ids, int ns, int *both);
OH_INTERNAL int neighbours_resolve(const int *const around_ids[2], const int *own_ids, int n, bool used, std::vector<int> around[2],
                                   std::vector<int> *srcs, int *side);
OH_INTERNAL int conv_sample_bytes(const OhConvert *cv, int bit_depth);
OH_INTERNAL int conv_check(const OhPicParams *p, const OhConvert *cv, size_t *bytes, std::string *why);
OH_INTERNAL int colour_check(const OhColour *col, std::string *why);
OH_INTERNAL int colour_build(const OhColour *col, int32_t *tab, int32_t *misc, std::string *why);
OH_INTERNAL int filter_check(const OhFilter *f, int bit_depth, std::string *why);
OH_INTERNAL void hist_derive(const uint32_t *bins, OhPlaneHist *out);
OH_INTERNAL int motion_check(const OhMotionSearch *ms, size_t n_centres, std::string *why);
OH_INTERNAL int warp_map_check(const OhWarp *w, std::string *why);
OH_INTERNAL int warp_check(const OhWarp *w, int bit_depth, std::string *why);
OH_INTERNAL int warp_image_check(const OhWarp *w, std::string *why);
OH_INTERNAL int lut_check(const OhLut *lut, int sbd, int dbd, int np, std::string *why);
OH_INTERNAL int grain_check(const OhGrain *g, int np, std::string *why);
OH_INTERNAL int remap_check(const OhRemap *r, std::string *why);
OH_INTERNAL bool remap_is_identity(const OhRemap *r);
struct PkPlane;
OH_INTERNAL int packing_check(const OhPacking *pk, std::string *why);
OH_INTERNAL int packing_geometry(const OhPacking *pk, const OhPicParams *packed, int full, PkPlane pl[2], OhPicParams *view, std::string *why);

#endif
