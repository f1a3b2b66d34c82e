// kw_conformance.hip — TEST INFRASTRUCTURE: the bodies of kw_conformance.hpp as gfx950 kernels behind one C entry point (libkwconf.so, built by build(); never part of
// libkai_core.so).  tests/test_gpu_kw_conformance.py runs the case table of tests/kw_conformance_cases.py through it on the MI355X.
// Include order: the product's (kai_core.hip / kai_handle.hpp).
#define KAI_SHARED_GPUS 1
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../kai-scheduler_amd/csrc/kai_host_prep.hpp"
#include "../../kai-scheduler_amd/csrc/kai_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_driver.hpp"
#include "../../kai-scheduler_amd/csrc/kai_victim_shard.hpp"
#include "../../kai-scheduler_amd/csrc/kai_delta.hpp"
#include "../../kai-scheduler_amd/csrc/kai_best_nodes.hpp"
#include "../../kai-scheduler_amd/csrc/kai_ops_apply.hpp"
#include "../../kai-scheduler_amd/csrc/kai_stale_gangs.hpp"
#include "kw_conformance.hpp"

#define KWC_X(id, name, iw, ow) __global__ void __launch_bounds__(1024) kwc_k_##name(const uint64_t* in, uint64_t* out, long long nw) { kwc::name(in, out, (int64_t)nw); }
KWC_CASES(KWC_X)
#undef KWC_X

// Runs one case: allocates, copies `in` and the preset `out` to the device, launches grid x block on the default stream, synchronises, copies `out` back, frees.
// Returns the first non-zero hipError_t, or 0; hipErrorInvalidValue without a launch for buffers too small for the shape.
extern "C" int kwc_run(int case_id, const void* in, size_t in_bytes, void* out, size_t out_bytes, int grid, int block) {
    if (!in || !out || !kwc::sizes_ok(case_id, in_bytes, out_bytes, grid, block)) return (int)hipErrorInvalidValue;
    if (case_id == 9 && !kwc::plan_setup_q_ok(in, in_bytes)) return (int)hipErrorInvalidValue;
    uint64_t *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc((void**)&d_in, in_bytes), e2;
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_out, out, out_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const long long nw = (long long)(in_bytes / 8);
        switch (case_id) {
#define KWC_X(id, name, iw, ow) case id: hipLaunchKernelGGL(kwc_k_##name, dim3(grid), dim3(block), 0, 0, d_in, d_out, nw); break;
            KWC_CASES(KWC_X)
#undef KWC_X
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    e2 = d_in ? hipFree(d_in) : hipSuccess; if (e == hipSuccess) e = e2;
    e2 = d_out ? hipFree(d_out) : hipSuccess; if (e == hipSuccess) e = e2;
    return (int)e;
}
