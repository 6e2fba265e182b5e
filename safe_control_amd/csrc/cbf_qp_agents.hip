// CBF-QP with per-agent robot and CBF parameters (sc_cbfqp_solve_batch_agents): the lane-per-QP kernel of cbf_qp_kernel.hpp
// instantiated with AGENTS = true, in a translation unit of its own.  One QP per lane at every B and K -- the cooperative and the
// compile-time-specialised kernels take their constants finished from the host and are not routed here.  Arithmetic is f64,
// storage f32 or f64; the 4-state models (Quad2D has no per-agent form).
#include "cbf_qp_kernel.hpp"
#include "sc_dispatch.hpp"

namespace sc {

// the caller (api.hip) has refused Quad2D and everything sc_cbfqp_solve_batch refuses
hipError_t cbfqp_agents_launch(const sc_cbfqp_params& p, const double* agent_params, long long B, int K, const void* X,
                               const void* u_ref, const void* obs, const int* n_obs, void* u_out, int* status, void* h_out,
                               hipStream_t stream) {
    const AgentQpArgs a{p, agent_params};
    const unsigned blocks = (unsigned)((B + 63) / 64);
    return dispatch_io(p.io_dtype, [&](auto tio) {
        using TIO = tag_t<decltype(tio)>;
        using TC = double;
        return dispatch_int_last<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D_C3BF,
                                 SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_UNICYCLE2D,
                                 SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF>(p.model_id, [&](auto model) {
            auto go = [&](auto kmax) {
                constexpr int KMAX = decltype(kmax)::value;
                // as launch_one: the staged obstacle rows, the assembled rows [K][3][64] and (KMAX > 0) the h stage [K][64]
                size_t lds = (p.obs_shared ? (size_t)K * 7 : (size_t)64 * K * 7) * sizeof(TIO);
                lds = ((lds + 15) & ~(size_t)15) + (size_t)K * 3 * 64 * sizeof(TC) + (KMAX > 0 ? (size_t)K * 64 * sizeof(TIO) : 0);
                return launch(cbfqp_kernel<TIO, TC, KMAX, decltype(model)::value, true>, blocks, 64, lds, stream, obs, X, u_ref, n_obs, B, K,
                              (int)p.obs_shared, u_out, status, h_out, a);
            };
            if (K <= 4) return go(int_tag<4>{});
            if (K <= 8) return go(int_tag<8>{});
            return go(int_tag<0>{});
        });
    });
}

}  // namespace sc
