// The fused closed loop with per-agent robot and CBF parameters (sc_tracking_rollout_batch_agents): the kernels and the dispatch
// of tracking_kernels.hpp instantiated with AGENTS = true, in a translation unit of their own so that the scalar unit builds as
// before.  Lane-per-agent and cooperative forms alike; arithmetic is f64, storage follows io_dtype.
#include <hip/hip_runtime.h>

#include "tracking_kernels.hpp"

namespace sc {

hipError_t tracking_agents_launch(const sc_tracking_params& p, const double* agent_params, long long B, int M, void* X,
                                  const void* wps, const int* n_wp, int* wp_index, int* sm, void* goal, void* table, void* u_last,
                                  int* ret, int* ret_step, void* tX, void* tU, hipStream_t stream) {
    TrackingAgentsArgs a;
    static_cast<sc_tracking_params&>(a) = p;
    a.agent_params = agent_params;
    return launch_track<true>(a, B, M, X, wps, n_wp, wp_index, sm, goal, table, u_last, ret, ret_step, tX, tU, stream);
}

}  // namespace sc
