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

namespace st {

// one 1024-lane workgroup per CU (the heap image of 2^20 leaves takes 128 KiB of LDS), as launch_canopy_heap
template <typename Src>
hipError_t launch_canopy_codes(const st_tree *t, const Src &src, int64_t n, DistSink out_d, MrcaSink out_m, Fault *fault,
                               hipStream_t stream)
{
    CodesParams C;
    C.codes = t->d_heap_codes;
    C.dist = t->d_heap_dist;
    C.nodes = t->d_nodes;
    C.depth = t->d_depth;
    C.stride = t->d_stride;
    C.n_nodes = t->n_nodes;
    C.levels = t->heap_levels;
    const size_t lds = heap_image_bytes(t->heap_levels);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_canopy_ilp_codes<Src>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    int64_t blocks = std::min<int64_t>((n + kCanopyBlock - 1) / kCanopyBlock, (int64_t)t->n_cu);
    blocks = std::max<int64_t>(blocks, 1);
    hipLaunchKernelGGL(k_canopy_ilp_codes<Src>, dim3((unsigned)blocks), dim3(kCanopyBlock), lds, stream, C, src, (long long)n,
                       out_d, out_m, fault);
    return hipGetLastError();
}

template hipError_t launch_canopy_codes<SrcContig>(const st_tree *, const SrcContig &, int64_t, DistSink, MrcaSink, Fault *, hipStream_t);
template hipError_t launch_canopy_codes<SrcContig32>(const st_tree *, const SrcContig32 &, int64_t, DistSink, MrcaSink, Fault *, hipStream_t);

}  // namespace st
