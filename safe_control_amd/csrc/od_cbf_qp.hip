// Optimal-decay CBF-QP, one problem per lane.
//   OptimalDecayCBFQP.solve_control_problem   position_control/optimal_decay_cbf_qp.py:131-158
// The row build and the 1 + 9 active-set solve live in od_qp.hpp, which the fused closed loop (tracking_od.hip) shares.
#include <hip/hip_runtime.h>

#include "od_qp.hpp"

namespace sc {

template <typename TIO> struct odv2;
template <> struct odv2<float> { using type = float2; };
template <> struct odv2<double> { using type = double2; };

template <typename TIO, typename TC, int MODEL>
__global__ __launch_bounds__(256) void odcbfqp_kernel(const sc_odcbfqp_params p, const long long B,
                                                      const TIO* __restrict__ X, const TIO* __restrict__ u_ref,
                                                      const TIO* __restrict__ obs, const int* __restrict__ has_obs,
                                                      TIO* __restrict__ u_out, TIO* __restrict__ omega_out,
                                                      int* __restrict__ status_out, TIO* __restrict__ h_out) {
    const long long agent = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (agent >= B) return;
    using V2 = typename odv2<TIO>::type;
    const V2 ur = reinterpret_cast<const V2*>(u_ref)[agent];
    const CbfConsts<TC> k = make_consts<TC>(p.qp);
    Agent<TC> ag;
    if constexpr (MODEL == SC_MODEL_QUAD2D) {                   // six states per row: [x, z, theta, vx, vz, theta_dot] (robots/quad2D.py:41-44)
        const TIO* r = X + agent * 6;
        ag = make_agent_m<TC, MODEL>(TC(r[0]), TC(r[1]), TC(r[2]), TC(r[3]), TC(r[4]));
    } else {
        const V2* Xv = reinterpret_cast<const V2*>(X) + agent * 2;
        const V2 xa = Xv[0], xb = Xv[1];
        ag = make_agent<TC>(TC(xa.x), TC(xa.y), TC(xb.x), TC(xb.y));
    }
    const TC r0 = TC(ur.x), r1 = TC(ur.y);
    const TC wr1 = TC(p.omega_ref[0]), wr2 = TC(p.omega_ref[1]);
    const TC p1 = TC(p.p_sb[0]), p2 = TC(p.p_sb[1]);
    constexpr bool REL2 = od_rel2<MODEL>::value;

    // ---- the row: A = dh g, b = dh f (optimal_decay_cbf_qp.py:138-146), e1, e2 -------------------
    OdRow<TC> row = od_row_none<TC>();
    const bool present = has_obs ? (has_obs[agent] != 0) : true;
    if (present) {
        TC o[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) o[f] = TC(obs[agent * 7 + f]);
        row = od_build_row<TC, MODEL>(ag, o, k);
    }
    const TC h = row.h;

    // ---- exact solve by KKT enumeration (od_qp.hpp) --------------------------------------------------
    TC u0, u1, w1, w2;
    const int st = od_solve<TC, REL2>(row, r0, r1, wr1, wr2, p1, p2, k, u0, u1, w1, w2);
    V2 uo; uo.x = TIO(u0); uo.y = TIO(u1);
    reinterpret_cast<V2*>(u_out)[agent] = uo;
    V2 wo; wo.x = TIO(w1); wo.y = TIO(w2);
    reinterpret_cast<V2*>(omega_out)[agent] = wo;
    status_out[agent] = st;
    if (h_out) h_out[agent] = present ? TIO(h) : TIO(0);
}

template <typename TIO, typename TC>
static hipError_t od_launch_model(const sc_odcbfqp_params& p, long long B, const void* X, const void* u_ref, const void* obs,
                                  const int* has_obs, void* u_out, void* w_out, int* status, void* h_out, hipStream_t stream) {
    const unsigned threads = 256, blocks = (unsigned)((B + threads - 1) / threads);
#define SC_OD(M)                                                                                                   \
    hipLaunchKernelGGL((odcbfqp_kernel<TIO, TC, M>), dim3(blocks), dim3(threads), 0, stream, p, B, (const TIO*)X, \
                       (const TIO*)u_ref, (const TIO*)obs, has_obs, (TIO*)u_out, (TIO*)w_out, status, (TIO*)h_out)
    switch (p.qp.model_id) {
        case SC_MODEL_DYNAMIC_UNICYCLE2D: SC_OD(SC_MODEL_DYNAMIC_UNICYCLE2D); break;
        case SC_MODEL_KINEMATIC_BICYCLE2D: SC_OD(SC_MODEL_KINEMATIC_BICYCLE2D); break;
        case SC_MODEL_KINEMATIC_BICYCLE2D_C3BF: SC_OD(SC_MODEL_KINEMATIC_BICYCLE2D_C3BF); break;
        case SC_MODEL_QUAD2D: SC_OD(SC_MODEL_QUAD2D); break;
        default: SC_OD(SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF); break;
    }
#undef SC_OD
    return hipGetLastError();
}

hipError_t odcbfqp_launch(const sc_odcbfqp_params& p, long long B, const void* X, const void* u_ref, const void* obs,
                          const int* has_obs, void* u_out, void* w_out, int* status, void* h_out, hipStream_t stream) {
    if (p.qp.io_dtype == SC_DTYPE_F32) {
        if (p.qp.compute_dtype == SC_DTYPE_F32)
            return od_launch_model<float, float>(p, B, X, u_ref, obs, has_obs, u_out, w_out, status, h_out, stream);
        return od_launch_model<float, double>(p, B, X, u_ref, obs, has_obs, u_out, w_out, status, h_out, stream);
    }
    return od_launch_model<double, double>(p, B, X, u_ref, obs, has_obs, u_out, w_out, status, h_out, stream);
}

}  // namespace sc
