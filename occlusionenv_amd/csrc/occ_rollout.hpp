// occ_rollout.hpp -- the PPO training loop's per-step and per-update bookkeeping (occ_ppo_act, occ_rollout_advance,
// occ_ppo_returns).  Part of the single translation unit occ_kernels.hip (included inside namespace occ; not a
// stand-alone header).
//
// The reference's training script (trainRL.py:189-247) does on the host, per env step: sample the action from the
// old policy (PPO.py:152-164), append reward and is_terminal to the buffer, add the reward to the episode's return and -
// when the episode ends - write one row of the training log and update the running reward.  Per update PPO.py:178-188
// turns the reward list into normalised Monte-Carlo returns.  Here each of the three is one launch on the batched env;
// tests/rollout_model.py states the same rules in numpy.

// ------------------------------------------------------------------------------------------
// (a) occ_ppo_act: action head, Gaussian sample and log-probability of n envs, and the step's row of the rollout buffer.
// One wave per env.  The lane partition (four features per lane), the per-lane expression and the reduction are those
// of occ_ppo_epoch_kernel's `consume` (occ_ppo.hpp), under the same contraction mode, and inv_var is formed as there: mean
// and quadratic term are what the first epoch of the update recomputes for the sample.  Only the additive constant is
// rounded differently (once, from double: the host code of occ_ppo_act says why).
// Row e depends on row e of the inputs only - not on n, not on the grid.
// ------------------------------------------------------------------------------------------
struct PpoActArgs {
    const float* feats; const float* w_a; const float* b_a; const float* noise;
    float action_std, inv_var, lp_const;
    int n;
    float* action; float* logprob; float* mean;           // (n,2), (n), (n,2) or null
    float* feat_buf; float* action_buf; float* logprob_buf;  // row t of (T,n,256) / (T,n,2) / (T,n), or all null
    long long row0;                                       // t * n
};

// `action = mean + noise * std` as torch forms it: the product is rounded, then the sum.  The function carries the
// contraction mode it is defined under into the kernel that inlines it (occ_episode.hpp on why __fmul_rn does not).
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) { return a * b + c; }
#pragma clang fp contract(fast)

constexpr int kActWaves = 4;  // envs per block

__global__ __launch_bounds__(64 * kActWaves) void occ_ppo_act_kernel(PpoActArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * kActWaves + wave;
    if (e >= A.n) return;  // (whole waves leave: the reductions below see 64 live lanes)
    const float4 wa0 = reinterpret_cast<const float4*>(A.w_a)[lane];
    const float4 wa1 = reinterpret_cast<const float4*>(A.w_a + kPpoFeat)[lane];
    const float4 f = reinterpret_cast<const float4*>(A.feats + (size_t)e * kPpoFeat)[lane];
    if (A.feat_buf) reinterpret_cast<float4*>(A.feat_buf + (size_t)(A.row0 + e) * kPpoFeat)[lane] = f;
    float d0 = f.x * wa0.x + f.y * wa0.y + f.z * wa0.z + f.w * wa0.w;
    float d1 = f.x * wa1.x + f.y * wa1.y + f.z * wa1.z + f.w * wa1.w;
    d0 = wave_sum_dpp(d0);
    d1 = wave_sum_dpp(d1);
    const float mean0 = d0 + A.b_a[0], mean1 = d1 + A.b_a[1];
    const float2 z = reinterpret_cast<const float2*>(A.noise)[e];
    const float a0 = mul_then_add(z.x, A.action_std, mean0), a1 = mul_then_add(z.y, A.action_std, mean1);
    const float e0 = a0 - mean0, e1 = a1 - mean1;
    const float lp = -0.5f * (e0 * e0 + e1 * e1) * A.inv_var + A.lp_const;  // log N(a; mean, var I), as `consume` writes it
    if (lane == 0) {
        reinterpret_cast<float2*>(A.action)[e] = make_float2(a0, a1);
        A.logprob[e] = lp;
        if (A.mean) reinterpret_cast<float2*>(A.mean)[e] = make_float2(mean0, mean1);
        if (A.action_buf) {
            reinterpret_cast<float2*>(A.action_buf)[A.row0 + e] = make_float2(a0, a1);
            A.logprob_buf[A.row0 + e] = lp;
        }
    }
}

// ------------------------------------------------------------------------------------------
// (b) occ_rollout_advance: after a step and its auto-reset.  Per env: the episode's return (f32, `current_ep_reward +=
// reward`) and length, and row t of the buffer's rewards / dones.  The envs whose code says that their episode ended (1 =
// done, 2 = time limit) leave one entry each in the episode ring IN ENV ORDER - entry k of all time goes to slot k % cap -
// and start again from zero.  Thread 0 then applies, in that order, the log's arithmetic (trainRL.py:231-237): the
// running reward in f32 (the first episode ever sets it; then 0.95f * running + 0.05f * return, both products rounded,
// then the sum) - kept per entry as well, the log's fourth column -, the f64 sums, the code counts.  One block of 1024 lanes, a round per 1024 envs, block_prefix_1024
// (occ_reset.hpp) for the ordered compaction; no atomics.
// ------------------------------------------------------------------------------------------
struct RolloutArgs {
    const float* reward; const uint8_t* done; const int* code;
    int n, cap;
    long long row0, timestep;            // t * n; the timestep the entries of this step carry
    float* rewards; float* dones;        // (T,n) each, or both null
    float* ep_return; int* ep_len;       // (n)
    int* ring_env; float* ring_return; int* ring_length; int* ring_code; long long* ring_timestep;  // (cap) each
    float* ring_running;                 // (cap): the running reward after the entry's episode (the log's fourth column)
    long long* n_episodes;               // (1)
    long long* code_counts;              // (2): episodes ended by done, by the time limit
    double* sums;                        // (2): sum of the completed returns, of their lengths
    float* running;                      // (1)
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(1024) void occ_rollout_advance_kernel(RolloutArgs a) {
    __shared__ int s_w[16];
    __shared__ float s_ret[1024];
    __shared__ int s_len[1024];
    __shared__ int s_code[1024];
    const int tid = threadIdx.x;
    const long long n0 = a.n_episodes[0];  // (thread 0 writes it after the last barrier below)
    long long nfin = 0;
    // thread 0's running state
    float running = 0.f;
    double sum_ret = 0.0, sum_len = 0.0;
    long long c1 = 0, c2 = 0;
    if (tid == 0) {
        running = a.running[0];
        sum_ret = a.sums[0];
        sum_len = a.sums[1];
        c1 = a.code_counts[0];
        c2 = a.code_counts[1];
    }
    for (int base = 0; base < a.n; base += 1024) {
        const int i = base + tid;
        bool f = false;
        float ret = 0.f;
        int len = 0, c = 0;
        if (i < a.n) {
            const float r = a.reward[i];
            c = a.code[i];
            f = c != 0;
            ret = a.ep_return[i] + r;
            len = a.ep_len[i] + 1;
            a.ep_return[i] = f ? 0.f : ret;
            a.ep_len[i] = f ? 0 : len;
            if (a.rewards) {
                a.rewards[a.row0 + i] = r;
                a.dones[a.row0 + i] = a.done[i] ? 1.0f : 0.0f;
            }
        }
        int tot;
        const int pos = block_prefix_1024(f, s_w, tid, tot);
        if (f) {
            s_ret[pos] = ret;
            s_len[pos] = len;
            s_code[pos] = c;
            // a later entry of this round that wraps onto the same slot wins: the earlier one is not written at all (the
            // rounds themselves are ordered by the barriers)
            if ((long long)pos + a.cap >= tot) {
                const int k = (int)((unsigned long long)(n0 + nfin + pos) % (unsigned long long)a.cap);
                a.ring_env[k] = i;
                a.ring_return[k] = ret;
                a.ring_length[k] = len;
                a.ring_code[k] = c;
                a.ring_timestep[k] = a.timestep;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int slot = (int)((unsigned long long)(n0 + nfin) % (unsigned long long)a.cap);
            for (int k = 0; k < tot; ++k) {
                const float rk = s_ret[k];
                running = (n0 + nfin + k == 0) ? rk : 0.95f * running + 0.05f * rk;
                a.ring_running[slot] = running;  // (in order: a later entry on the same slot overwrites)
                slot = slot + 1 == a.cap ? 0 : slot + 1;
                sum_ret += (double)rk;
                sum_len += (double)s_len[k];
                if (s_code[k] == 1) c1 += 1; else c2 += 1;
            }
        }
        nfin += tot;
    }
    if (tid == 0 && nfin > 0) {
        a.running[0] = running;
        a.sums[0] = sum_ret;
        a.sums[1] = sum_len;
        a.code_counts[0] = c1;
        a.code_counts[1] = c2;
        a.n_episodes[0] = n0 + nfin;
    }
}

// ------------------------------------------------------------------------------------------
// (c) occ_ppo_returns: the discounted returns of PPO.py:178-185 per env, `running = r + (gamma * running) * not_done`
// with three rounded f32 operations as ppo.mc_returns states it, then mean and unbiased standard deviation of all
// M = T n returns in f64 (two passes: the mean, then the squared deviations) and the normalised returns
// (ret - (float)mean) / ((float)std + 1e-7f).  One block: thread k adds elements k, k + 1024, ... in index order and the
// 1024 partial sums are folded in halves - an order fixed by M alone.
// ------------------------------------------------------------------------------------------
struct ReturnsArgs {
    const float* rewards; const float* dones;  // (T,n)
    int T, n;
    float gamma;
    float* out;     // (T n): the normalised returns (holds the raw ones in between)
    float* raw;     // (T n) or null: the returns before the normalisation
    double* stats;  // (2): mean, std
};

__device__ __forceinline__ double block_sum_1024(double v, double* s, int tid) {
    __syncthreads();  // s reuse
    s[tid] = v;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (tid < h) s[tid] += s[tid + h];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(1024) void occ_ppo_returns_kernel(ReturnsArgs a) {
    __shared__ double s_sum[1024];
    const int tid = threadIdx.x;
    const long long M = (long long)a.T * a.n;
    for (int e = tid; e < a.n; e += 1024) {
        float running = 0.f;
        for (int t = a.T - 1; t >= 0; --t) {
            const long long i = (long long)t * a.n + e;
            const float not_done = 1.0f - a.dones[i];
            running = a.rewards[i] + (a.gamma * running) * not_done;
            a.out[i] = running;
            if (a.raw) a.raw[i] = running;
        }
    }
    __syncthreads();  // (one block: the barrier orders its global stores before the loads below)
    double acc = 0.0;
    for (long long i = tid; i < M; i += 1024) acc += (double)a.out[i];
    const double mean = block_sum_1024(acc, s_sum, tid) / (double)M;
    acc = 0.0;
    for (long long i = tid; i < M; i += 1024) {
        const double d = (double)a.out[i] - mean;
        acc += d * d;
    }
    const double sd = sqrt(block_sum_1024(acc, s_sum, tid) / (double)(M - 1));
    if (tid == 0) {
        a.stats[0] = mean;
        a.stats[1] = sd;
    }
    const float mf = (float)mean, den = (float)sd + 1e-7f;
    for (long long i = tid; i < M; i += 1024) a.out[i] = (a.out[i] - mf) / den;
}
#pragma clang fp contract(fast)
