// Trunk kernels with 256 filters, v2 (pre-activation / squeeze-excite) nets (trunk_variants.h).
#include "trunk_variants.h"

namespace gznn {

KernelChoice trunk_variant_f256_v2(int pt, int v, int precision) {
    switch (pt) {
        case 4: return variants<256, 4, true>(v, precision);
        case 7: return variants<256, 7, true>(v, precision);
        case 11: return variants<256, 11, true>(v, precision);
        default: return KernelChoice{};
    }
}

}  // namespace gznn
