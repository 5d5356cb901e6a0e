// occ_episode.hpp -- episode bookkeeping of the batched controller evaluation (occ_episode_advance).
// Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a stand-alone header).

// ------------------------------------------------------------------------------------------
// One launch after every step does what the reference's evaluation loops do on the host (test.py:92-255,
// iterator.py:104-204): the controller's update of the action, the NaN test of the raw gradient, the reward traces, the
// `finished` / step-cap test - and it freezes the envs that are through (active = 0, skip = 1: the next step's launch
// leaves their rows alone, OccScene.skip).  One lane per env; tests/episode_model.py is this rule in numpy.
// ------------------------------------------------------------------------------------------
struct EpisodeArgs {
    const uint8_t* done; const float* reward; const float* full_reward;  // this step's outputs, (n)
    const float* grad; const float* pred; const float* noise;            // (n,2) each; only the rule's own is read
    int rule; float lr; int step, max_step, n;
    float* action; int* active; int* skip; int* iterations; uint8_t* finished; int* nan_steps;
    float* tr_reward; float* tr_full;  // (max_step, n) traces or null
    int* report;
};

// torch rounds the product and the sum of `action += lr * grad` separately, so nothing below may be contracted into a
// fused multiply-add.  HIP's __fmul_rn / __fadd_rn do not see to that: they are inline `*` and `+` that carry the contract
// flag of the header they are defined in, and the pair was fused even with contraction off here (measured: one ulp off
// the model).  Plain operators under the pragma are what holds.
#pragma clang fp contract(off)
// (One block: the launch is a few hundred lanes of a dozen loads each, and the count of the envs still active comes out
// of one block reduction - no zeroing launch, no atomics; envs beyond 1024 take further rounds of the same block.)
__global__ __launch_bounds__(1024) void occ_episode_kernel(EpisodeArgs a) {
    __shared__ int s_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int still = 0;
    for (int e = tid; e < a.n; e += blockDim.x) {
        if (a.active[e] == 0) continue;  // frozen: nothing read, nothing written
        bool nan_step = false;
        float a0 = a.action[2 * e], a1 = a.action[2 * e + 1];
        if (a.rule == OCC_EPISODE_GRADIENT) {
            const float g0 = a.grad[2 * e], g1 = a.grad[2 * e + 1];
            nan_step = (g0 != g0) || (g1 != g1);
            if (!nan_step) {  // action += lr * action.grad: the product is rounded, then the sum (no fused multiply-add)
                a0 = a0 + a.lr * g0;
                a1 = a1 + a.lr * g1;
            }
        } else if (a.rule == OCC_EPISODE_RANDOM) {
            a0 = a0 + a.lr * a.noise[2 * e];
            a1 = a1 + a.lr * a.noise[2 * e + 1];
        } else if (a.rule == OCC_EPISODE_MODEL) {
            a0 = -a.lr * a.pred[2 * e];
            a1 = -a.lr * a.pred[2 * e + 1];
        } else {
            a0 = a.pred[2 * e];
            a1 = a.pred[2 * e + 1];
        }
        bool freeze = false;
        if (nan_step) {
            a.nan_steps[e] += 1;  // `continue` at iterator.py:118-120: no update, no trace row, no finished test
        } else {
            a.action[2 * e] = a0;
            a.action[2 * e + 1] = a1;
            if (a.tr_reward) a.tr_reward[(size_t)a.step * a.n + e] = a.reward[e];
            if (a.tr_full) a.tr_full[(size_t)a.step * a.n + e] = a.full_reward[e];
            if (a.done[e]) {
                a.finished[e] = 1;
                freeze = true;
            }
        }
        if (a.step == a.max_step - 1) freeze = true;  // the cap, on a NaN step as well
        if (freeze) {
            a.iterations[e] = a.step + 1;
            a.active[e] = 0;
            a.skip[e] = 1;
        } else {
            still += 1;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) still += __shfl_down(still, d, 64);
    if (lane == 0) s_cnt[wave] = still;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += s_cnt[w];
        a.report[0] = tot;
    }
}
// (this header is included last: what follows it in occ_kernels.hip is the extern "C" host code, back on the build's default)
#pragma clang fp contract(fast)
