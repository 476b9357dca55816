// Library introspection entry points of the C ABI (include/snap_hip.h).
#include "common.h"

#include <cstddef>

// The Python binding derives its struct classes from the header's text; these pin what the
// compiler makes of the same text (tests/test_host_logic.py asserts the same numbers).
static_assert(sizeof(SnapConvDesc) == 76 && offsetof(SnapConvDesc, tile_hint) == 72, "SnapConvDesc layout");
static_assert(sizeof(SnapConvExtras) == 200 && offsetof(SnapConvExtras, gnb_mode) == 192, "SnapConvExtras layout");
static_assert(sizeof(SnapLiftDesc) == 92 && offsetof(SnapLiftDesc, tune_flags) == 88, "SnapLiftDesc layout");
static_assert(sizeof(SnapPackItem) == 32 && offsetof(SnapPackItem, block_begin) == 28, "SnapPackItem layout");
static_assert(sizeof(SnapWstdItem) == 40 && offsetof(SnapWstdItem, reserved) == 36, "SnapWstdItem layout");
static_assert(sizeof(SnapAdamItem) == 48 && offsetof(SnapAdamItem, block_begin) == 40, "SnapAdamItem layout");

extern "C" int snap_abi_version(void) { return SNAP_ABI_VERSION; }

extern "C" const char* snap_build_arch(void) { return "gfx950"; }

extern "C" const char* snap_status_string(int status) {
  switch (status) {
    case SNAP_OK: return "ok";
    case SNAP_ERR_BAD_SHAPE: return "bad or inconsistent shape";
    case SNAP_ERR_UNSUPPORTED: return "unsupported option";
    case SNAP_ERR_NULL: return "required pointer is NULL";
    case SNAP_ERR_LAUNCH: return "HIP launch error";
    case SNAP_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown status";
  }
}
