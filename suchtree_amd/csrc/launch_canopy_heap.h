// launch_canopy_heap.h -- launch_heap_family: the host launcher of the two heap-family kernels (k_canopy_ilp_heap in
// launch_canopy.hip, k_canopy_ilp_codes in launch_canopy_codes.hip).  Include after the kernel's header, st_tree.h and <algorithm>.
#pragma once

namespace st {

// `kern` over `lines` (the handle's heap lines or heap codes): one 1024-lane workgroup per CU (the heap image of 2^20 leaves
// takes 128 KiB of LDS)
template <typename Word, typename Src>
static hipError_t launch_heap_family(void (*kern)(HeapParamsT<Word>, Src, long long, DistSink, MrcaSink, Fault *),
                                     decltype(HeapParamsT<Word>::lines) lines, const st_tree *t, const Src &src, int64_t n,
                                     DistSink out_d, MrcaSink out_m, Fault *fault, hipStream_t stream)
{
    HeapParamsT<Word> H;
    H.lines = lines;
    H.dist = t->d_heap_dist;
    H.nodes = t->d_nodes;
    H.depth = t->d_depth;
    H.stride = t->d_stride;
    H.n_nodes = t->n_nodes;
    H.levels = t->heap_levels;
    const size_t lds = heap_image_bytes(t->heap_levels);
    if (lds > 64 * 1024) {      // dynamic LDS above 64 KiB has to be granted per kernel
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    int64_t blocks = std::min<int64_t>((n + kCanopyBlock - 1) / kCanopyBlock, (int64_t)t->n_cu);
    blocks = std::max<int64_t>(blocks, 1);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kCanopyBlock), lds, stream, H, src, (long long)n, out_d, out_m, fault);
    return hipGetLastError();
}

}  // namespace st
