// CBF-QP with per-agent robot and CBF parameters (sc_cbfqp_solve_batch_agents): the lane-per-QP kernel of cbf_qp_kernel.hpp
// instantiated with AGENTS = true, in a translation unit of its own.  One QP per lane at every B and K -- the cooperative and the
// compile-time-specialised kernels take their constants finished from the host and are not routed here.  Arithmetic is f64,
// storage f32 or f64; the 4-state models (Quad2D has no per-agent form).
#include "cbf_qp_kernel.hpp"

namespace sc {

template <typename TIO, int KMAX, int MODEL>
static hipError_t launch_agents_one(const AgentQpArgs& a, long long B, int K, const void* X, const void* u_ref, const void* obs,
                                    const int* n_obs, void* u_out, int* status, void* h_out, hipStream_t stream) {
    using TC = double;
    const unsigned blocks = (unsigned)((B + 63) / 64);
    // as launch_one: the staged obstacle rows, the assembled rows [K][3][64] and (KMAX > 0) the h stage [K][64]
    size_t lds = (a.qp.obs_shared ? (size_t)K * 7 : (size_t)64 * K * 7) * sizeof(TIO);
    lds = ((lds + 15) & ~(size_t)15) + (size_t)K * 3 * 64 * sizeof(TC) + (KMAX > 0 ? (size_t)K * 64 * sizeof(TIO) : 0);
    auto kern = cbfqp_kernel<TIO, TC, KMAX, MODEL, true>;
    if (lds > 64 * 1024) {                                  // dynamic LDS above 64 KiB needs the attribute (per device: set per call)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, stream, (const TIO*)obs, (const TIO*)X, (const TIO*)u_ref, n_obs, B, K,
                       (int)a.qp.obs_shared, (TIO*)u_out, status, (TIO*)h_out, a);
    return hipGetLastError();
}

template <typename TIO, int MODEL>
static hipError_t launch_agents_k(const AgentQpArgs& a, long long B, int K, const void* X, const void* u_ref, const void* obs,
                                  const int* n_obs, void* u_out, int* status, void* h_out, hipStream_t stream) {
    if (K <= 4) return launch_agents_one<TIO, 4, MODEL>(a, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
    if (K <= 8) return launch_agents_one<TIO, 8, MODEL>(a, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
    return launch_agents_one<TIO, 0, MODEL>(a, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
}

template <typename TIO>
static hipError_t launch_agents_model(const AgentQpArgs& a, long long B, int K, const void* X, const void* u_ref, const void* obs,
                                      const int* n_obs, void* u_out, int* status, void* h_out, hipStream_t stream) {
#define SC_AGENTS_MODEL(ID) return launch_agents_k<TIO, ID>(a, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream)
    switch (a.qp.model_id) {
        case SC_MODEL_DYNAMIC_UNICYCLE2D: SC_AGENTS_MODEL(SC_MODEL_DYNAMIC_UNICYCLE2D);
        case SC_MODEL_KINEMATIC_BICYCLE2D: SC_AGENTS_MODEL(SC_MODEL_KINEMATIC_BICYCLE2D);
        case SC_MODEL_KINEMATIC_BICYCLE2D_C3BF: SC_AGENTS_MODEL(SC_MODEL_KINEMATIC_BICYCLE2D_C3BF);
        case SC_MODEL_SINGLE_INTEGRATOR2D: SC_AGENTS_MODEL(SC_MODEL_SINGLE_INTEGRATOR2D);
        case SC_MODEL_DOUBLE_INTEGRATOR2D: SC_AGENTS_MODEL(SC_MODEL_DOUBLE_INTEGRATOR2D);
        case SC_MODEL_UNICYCLE2D: SC_AGENTS_MODEL(SC_MODEL_UNICYCLE2D);
        default: SC_AGENTS_MODEL(SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF);
    }
#undef SC_AGENTS_MODEL
}

// the caller (api.hip) has refused Quad2D and everything sc_cbfqp_solve_batch refuses
hipError_t cbfqp_agents_launch(const sc_cbfqp_params& p, const double* agent_params, long long B, int K, const void* X,
                               const void* u_ref, const void* obs, const int* n_obs, void* u_out, int* status, void* h_out,
                               hipStream_t stream) {
    const AgentQpArgs a{p, agent_params};
    if (p.io_dtype == SC_DTYPE_F32)
        return launch_agents_model<float>(a, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
    return launch_agents_model<double>(a, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
}

}  // namespace sc
