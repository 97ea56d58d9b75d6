// launch_canopy_codes.hip -- translation unit of k_canopy_ilp_codes (kernels_canopy_codes.h): the predicated kernel on heap
// codes, for the two explicit pair sources, behind launch_canopy_codes<Src> (called from launch_canopy.hip: launch_canopy_t).
// A unit of its own so that the units of launch_canopy.hip compile to what they were.  Built for gfx950 only:
// hipcc --offload-arch=gfx950 -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#define ST_LAUNCH_UNIT 1
#include "device_common.h"
#include "pair_math.h"
#include "tree_prep.h"
#include "st_tree.h"
#include "launch_decl.h"
#include "launch_policy.h"
#include "kernels_canopy_codes.h"
#include "launch_canopy_heap.h"

namespace st {

template <typename Src>
hipError_t launch_canopy_codes(const st_tree *t, const Src &src, int64_t n, DistSink out_d, MrcaSink out_m, Fault *fault,
                               hipStream_t stream)
{
    return launch_heap_family(k_canopy_ilp_codes<Src>, t->d_heap_codes, t, src, n, out_d, out_m, fault, stream);
}

template hipError_t launch_canopy_codes<SrcContig>(const st_tree *, const SrcContig &, int64_t, DistSink, MrcaSink, Fault *, hipStream_t);
template hipError_t launch_canopy_codes<SrcContig32>(const st_tree *, const SrcContig32 &, int64_t, DistSink, MrcaSink, Fault *, hipStream_t);

}  // namespace st
