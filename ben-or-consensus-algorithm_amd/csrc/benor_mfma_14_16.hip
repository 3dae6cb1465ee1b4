// Matrix-core kernel instantiations W = 14..16 (benor_mfma.h: KIND 0..2 x both
// tile parities each), split over four units so the unrolled instantiations
// build in parallel.
#include "benor_mfma.h"

namespace benor {
template hipError_t launch_mfma<14>(const KParams &, int, hipStream_t);
template int mfma_sure_blocks_per_cu<14>(const KParams &);
template hipError_t launch_mfma<15>(const KParams &, int, hipStream_t);
template int mfma_sure_blocks_per_cu<15>(const KParams &);
template hipError_t launch_mfma<16>(const KParams &, int, hipStream_t);
template int mfma_sure_blocks_per_cu<16>(const KParams &);
}  // namespace benor
