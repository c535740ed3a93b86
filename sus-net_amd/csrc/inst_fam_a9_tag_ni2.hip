// the byte-parallel family: 9 agents, TAG (two imposters) -- one translation unit of the parallel build (tools/gen_family.py, susnet_family.h)
#include "susnet_family.h"
namespace susnet {
SUSNET_FAMILY_INSTANTIATE(9, SUSNET_VARIANT_TAGGING, 1, 2)
SUSNET_FAMILY_INSTANTIATE(9, SUSNET_VARIANT_TAGGING, 0, 2)
}
