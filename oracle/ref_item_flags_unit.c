/* ref_harness.c once more, with ref_set_item_flags(): the candidate flags lc->na of every intra block come from OhIntra.avail
 * instead of the single-slice derivation (oracle/Makefile: ref_flags).  TEST INFRASTRUCTURE ONLY. */
#define OH_REF_ITEM_FLAGS 1
#include "ref_harness.c"
