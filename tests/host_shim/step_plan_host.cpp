// Host build of citylearn_amd/csrc/cl_plan.h: the step path's kernel selection on a CPU (TEST HARNESS ONLY; the library launches the plan).
// g++ -std=c++17 -O1 -shared -fPIC step_plan_host.cpp -o libstep_plan_host.so
#include "../../citylearn_amd/csrc/cl_plan.h"

// plan_step + plan_name for one call: returns the plan_step code; `name` (CL_KERNEL_NAME_LEN bytes) gets the kernel_name of an accepted call,
// `err` (512 bytes) the cl_last_error message of a refused one; `geom` = grid x, grid y, block, LDS bytes, nw, b_chunk, n_chunks, fused_finish.
extern "C" int host_plan_step(const cl_dims* dims, const cl_tuning* tuning, long long act_stride_env, int flex, int obs, int obs_lean_ok, int obs_pitch,
                              char* name, char* err, long long* geom) {
    cl_tuning tun = tuning ? *tuning : cl_tuning{};
    tun.kernel_name = name;
    g_err[0] = 0;
    StepPlan p;
    const int rc = plan_step(p, *dims, tun, act_stride_env, flex != 0, obs != 0, obs_lean_ok != 0, obs_pitch);
    snprintf(err, 512, "%s", g_err);
    if (rc != CL_OK) return rc;
    plan_name(p, tun);
    const long long g[8] = {p.grid_x, p.grid_y, p.block, (long long)p.lds, p.nw, p.b_chunk, p.n_chunks, p.fused_finish};
    for (int i = 0; i < 8; ++i) geom[i] = g[i];
    return rc;
}
