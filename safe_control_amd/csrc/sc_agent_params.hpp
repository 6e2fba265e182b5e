// Per-agent robot and CBF parameters (include/safe_control_amd.h: SC_AP_*): where the `_agents` instantiations of the CBF-QP and
// fused-loop kernels get the quantities that the scalar instantiations read from their launch-uniform struct.
//
// The table is [SC_AGENT_PARAM_COLS][B] doubles, agents contiguous.  A kernel patches an agent's columns into a copy of the
// launch-uniform sc_cbfqp_params and hands that to make_consts (sc_models.hpp): the derived constants are formed by the very
// expressions of the scalar path, in double, before the cast to the compute type -- a table whose rows equal the struct gives the
// struct's bits.  The loads happen once per launch, before the step loop; the constants live in registers from there.
//
// Cooperative kernels (G lanes per agent): every lane of a group loads its agent's columns itself.  The G lanes present the same
// address, which the memory pipeline serves as one access; moving the values from one lane through the DPP group moves of
// sc_group.hpp instead would cost two v_mov_dpp per column and lane on top of the same ten load instructions (a load is issued per
// wave, not per lane), and these ten loads sit next to the state / waypoint loads of the kernel's prologue, in their latency shadow.
#pragma once
#include <type_traits>

#include "sc_models.hpp"

namespace sc {

// kernel argument of the per-agent CBF-QP solve, in the slot where the scalar kernel takes its finished CbfConsts
struct AgentQpArgs {
    sc_cbfqp_params qp;             // the launch-uniform fields (dt, cbf_mode, rear_ax_dist, mass); the tabled ones are not read
    const double* table;            // [SC_AGENT_PARAM_COLS][B]
};

// kernel argument of the per-agent fused loop, in the slot of sc_tracking_params
struct TrackingAgentsArgs : sc_tracking_params {
    const double* agent_params;     // [SC_AGENT_PARAM_COLS][B]
};

template <bool AGENTS> using TrackingArgs = std::conditional_t<AGENTS, TrackingAgentsArgs, sc_tracking_params>;
template <bool AGENTS, typename TC> using CbfQpArgs = std::conditional_t<AGENTS, AgentQpArgs, CbfConsts<TC>>;

__device__ __forceinline__ double agent_col(const double* __restrict__ table, const int col, const long long B, const long long agent) {
    return table[(size_t)col * (size_t)B + (size_t)agent];
}

// sc_cbfqp_params of one agent: the launch-uniform struct with the agent's columns in place of its own
__device__ __forceinline__ sc_cbfqp_params agent_qp(const sc_cbfqp_params& uniform, const double* __restrict__ table,
                                                    const long long B, const long long agent) {
    sc_cbfqp_params q = uniform;
    q.robot_radius = agent_col(table, SC_AP_RADIUS, B, agent);
    q.alpha1 = agent_col(table, SC_AP_ALPHA1, B, agent);
    q.alpha2 = agent_col(table, SC_AP_ALPHA2, B, agent);
    q.u_min[0] = agent_col(table, SC_AP_U_MIN0, B, agent);
    q.u_min[1] = agent_col(table, SC_AP_U_MIN1, B, agent);
    q.u_max[0] = agent_col(table, SC_AP_U_MAX0, B, agent);
    q.u_max[1] = agent_col(table, SC_AP_U_MAX1, B, agent);
    return q;
}

// the constants of the solve kernels: handed over finished by the scalar launch, built from the agent's columns by the per-agent one
template <typename TC>
__device__ __forceinline__ const CbfConsts<TC>& solve_consts(const CbfConsts<TC>& k, long long, long long) { return k; }
template <typename TC>
__device__ __forceinline__ CbfConsts<TC> solve_consts(const AgentQpArgs& a, const long long B, const long long agent) {
    return make_consts<TC>(agent_qp(a.qp, a.table, B, agent));
}

// the controller parameters of the fused loop
__device__ __forceinline__ const sc_cbfqp_params& track_qp(const sc_tracking_params& p, long long, long long) { return p.qp; }
__device__ __forceinline__ sc_cbfqp_params track_qp(const TrackingAgentsArgs& p, const long long B, const long long agent) {
    return agent_qp(p.qp, p.agent_params, B, agent);
}

// reached_threshold, v_max, v_min of the fused loop
struct TrackScalars { double reached, v_max, v_min; };
__device__ __forceinline__ TrackScalars track_scalars(const sc_tracking_params& p, long long, long long) {
    return TrackScalars{p.reached_threshold, p.v_max, p.v_min};
}
__device__ __forceinline__ TrackScalars track_scalars(const TrackingAgentsArgs& p, const long long B, const long long agent) {
    return TrackScalars{agent_col(p.agent_params, SC_AP_REACHED, B, agent), agent_col(p.agent_params, SC_AP_V_MAX, B, agent),
                        agent_col(p.agent_params, SC_AP_V_MIN, B, agent)};
}

}  // namespace sc
