// fragments_plan.cpp -- the host helper of the fragment support (fragments_plan.hpp).  Nothing here touches the device.
#include "fragments_plan.hpp"
#include "../../include/pantax_hip.h"

static_assert(ptx::FRG_N_CLASSES == PANTAX_HIP_FRAGMENT_CLASSES, "the class order of species_out");

extern "C" int pantax_hip_fragment_key(const char *id, uint64_t len, uint64_t *key_out, uint8_t *tag_out) {
    if (!id || !key_out || !tag_out) return PANTAX_HIP_E_INVALID;
    ptx::fragment_key(id, len, *key_out, *tag_out);
    return 0;
}
