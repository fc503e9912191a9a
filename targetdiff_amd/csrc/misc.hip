// Small per-ligand-atom kernels of one reverse-diffusion step (gfx950):
//   * head_kernel       v_inference = Linear -> ShiftedSoftplus -> Linear on ligand rows
//                       (models/molopt_score_model.py:307-311,351-352; models/common.py:156-162)
//   * posterior_kernel  Gaussian + categorical posterior and Gumbel-max draw
//                       (models/molopt_score_model.py:673-685 and the helpers cited in targetdiff_hip.h)
//   * renoise_kernel    the forward-process step of a sampling time program (no seam in the reference; its pieces are :577-588, :371-381)
//   * center kernels    center_pos(mode='protein') (models/molopt_score_model.py:110-120)
// The reference spends ~40 tiny launches and two host syncs per step here; each is one launch.
#include "td_device.h"
#include "td_internal.h"

constexpr int HEAD_ATOMS = 8;

__global__ __launch_bounds__(128) void head_kernel(TdHead hd, const float *__restrict__ h,
                                                   const float4 *__restrict__ x4,
                                                   const int32_t *__restrict__ lig_node, int64_t Nl, int C,
                                                   float *__restrict__ pred_pos, float *__restrict__ pred_v,
                                                   float *__restrict__ lig_h) {
    __shared__ float s_h[HEAD_ATOMS][TD_H];
    __shared__ float s_y[HEAD_ATOMS][TD_H];
    const int n = threadIdx.x;
    const int64_t a0 = (int64_t)blockIdx.x * HEAD_ATOMS;
    for (int a = 0; a < HEAD_ATOMS; ++a) {
        const int64_t at = a0 + a;
        float v = 0.f;
        if (at < Nl) {
            const int64_t p = lig_node ? (int64_t)lig_node[at] : at;     // nullptr: free-standing rows (return_all)
            v = h[p * TD_H + n];
            if (lig_h) lig_h[at * TD_H + n] = v;
            if (n < 3 && x4) {
                const float4 xp = x4[p];
                pred_pos[at * 3 + n] = n == 0 ? xp.x : (n == 1 ? xp.y : xp.z);
            }
        }
        s_h[a][n] = v;
    }
    __syncthreads();
    float acc[HEAD_ATOMS];
    const float b0 = hd.b0[n];
#pragma unroll
    for (int a = 0; a < HEAD_ATOMS; ++a) acc[a] = b0;
#pragma unroll 16        // sixteen weight loads in flight
    for (int k = 0; k < TD_H; ++k) {
        const float wv = hd.W0T[k * TD_H + n];
#pragma unroll
        for (int a = 0; a < HEAD_ATOMS; ++a) acc[a] = fmaf(wv, s_h[a][k], acc[a]);
    }
#pragma unroll
    for (int a = 0; a < HEAD_ATOMS; ++a) {
        const float xv = acc[a];
        const float sp = xv > 20.f ? xv : log1pf(expf(xv));          // F.softplus (beta 1, threshold 20)
        s_y[a][n] = sp - 0.69314718055994531f;                      // ShiftedSoftplus: - log(2)
    }
    __syncthreads();
    // second Linear: 128 -> C (C <= 16).  thread (a, cc) = (n / 16, n % 16)
    const int a = n >> 4, cc = n & 15;
    if (cc < C && a0 + a < Nl) {
        float o = hd.b2[cc];
#pragma unroll 16
        for (int k = 0; k < TD_H; ++k) o = fmaf(hd.W2T[k * TD_MAXC + cc], s_y[a][k], o);
        pred_v[(a0 + a) * C + cc] = o;
    }
}

int td_launch_head(const TdHead &hd, const float *h, const float4 *x4, const int32_t *lig_node, int64_t Nl,
                   int classes, float *pred_pos, float *pred_v, float *lig_h, hipStream_t s) {
    if (Nl == 0) return TD_OK;
    head_kernel<<<dim3((unsigned)((Nl + HEAD_ATOMS - 1) / HEAD_ATOMS)), dim3(128), 0, s>>>(
        hd, h, x4, lig_node, Nl, classes, pred_pos, pred_v, lig_h);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

// ------------------------------------------------------------------------------------------ posterior
// one ligand atom of the posterior update; `a` names its inputs and outputs (TdStepArgs, td_internal.h).  a.pos / a.v may alias
// a.pos_next / a.v_next and a.pos_cur / a.v_cur (the in-place form of td_session_step): every input of the atom is read before its
// outputs are written, and atoms do not read each other.  pos_cur / v_cur (optional): second copies of x_{t-1} / v_{t-1} (the
// trajectory slot and the current state of td_session_step); v_frozen: pos_only, v_next = the input type.
// FIXED (scaffold-constrained sampling): atoms flagged in fixed_mask do not take the posterior draw but a forward-diffused
// copy of their known state (fixed_pos [N_l,3] centred, fixed_v [N_l]) at level t - 1, made from this step's own draws for the atom:
//   t > 0:  x' = sqrt(abar[t-1]) x0 + sqrt(1 - abar[t-1]) eps,   v' = argmax_c(gumbel(u_c) + log q(v_{t-1} = c | v0))   (q_v_sample)
//   t == 0: x' = x0, v' = v0.   a.log_post receives that log q (t == 0: the clamped log one-hot), a.log_v0 the model's as ever.
// FIXED = false compiles to the code without the feature.
// PROG (time programs): the step goes from level t to any lower level s; its coefficients come from the slot's row
// `a.prow` (TD_PROG_ROW floats, td_prog_col order, built on the host by TimeProgram.tables) instead of the per-t tables, "t == 0" reads
// "s is clean data" (prow[TD_PROG_LAST]), and the known atoms' level is s (prow[TD_PROG_ABAR_TO], log_ca / log_1mca of s).  The network
// still ran at t: model_mean_type 'noise' takes rc[t] / rm1[t].  PROG = false compiles to the code without the feature.
// GUIDED (clash guidance): the step uses x0' = fl32(x0 + a.x0_shift[atom]) -- one rounded add on the x0 the line below
// forms, on every step, the last included -- in place of x0.  Known atoms ignore it (they are overwritten).  GUIDED = false compiles to the
// code without the feature.
template <bool FIXED, bool PROG, bool GUIDED>
__device__ __forceinline__ void td_posterior_atom(const TdSchedules &sc, const TdStepArgs &a, int64_t at) {
    const int C = a.C;
    const float *prow = a.prow;
    const int g = td_find_graph(a.lptr, a.B, (int)at);
    int t = a.t[g];
    t = t < 0 ? 0 : (t >= a.T ? a.T - 1 : t);
    // ---- positions: mean = c0[t] x0 + ct[t] x_t ; x_{t-1} = mean + [t != 0] exp(0.5 logvar[t]) eps  (:673-679)
    const bool last = PROG ? prow[TD_PROG_LAST] != 0.f : t == 0;          // the step ends on clean data: no noise, known atoms as they are
    const float c0 = PROG ? prow[TD_PROG_C0] : sc.c0[t], ct = PROG ? prow[TD_PROG_CT] : sc.ct[t];
    const float sd = last ? 0.f : expf(0.5f * (PROG ? prow[TD_PROG_LOGVAR] : sc.logvar[t]));
    float xn[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)       // three products, two sums, each rounded on its own -- PyTorch's eager arithmetic (:376, :679), and the
                                      // same bits in every kernel this function is inlined into (no compiler-chosen FMA contraction)
    {
        const float xt = a.pos[at * 3 + d];
        // model_mean_type 'noise' (:412-416, :663-666): the network's output is x_t + eps; x0 = rc[t] x_t - rm1[t] eps
        float x0 = td_x0_of_output(sc.rc, sc.rm1, t, a.mean_type, a.pred_pos[at * 3 + d], xt);
        if (GUIDED) x0 = td_add_rn(x0, a.x0_shift[at * 3 + d]);
        xn[d] = td_add_rn(td_add_rn(td_mul_rn(c0, x0), td_mul_rn(ct, xt)), td_mul_rn(sd, a.noise[at * 3 + d]));
    }
    const int vt = (int)a.v[at];
    const bool known = FIXED && a.fixed_mask[at] != 0;
    if (FIXED && known) {
        // the products and the sum each rounded on their own, as torch's eager a.sqrt() * x0 + (1 - a).sqrt() * eps (:577-588)
        const float ab = PROG ? prow[TD_PROG_ABAR_TO] : sc.abar[t - 1 < 0 ? 0 : t - 1];
        const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float x0 = a.fixed_pos[at * 3 + d];
            xn[d] = last ? x0 : td_add_rn(td_mul_rn(sa, x0), td_mul_rn(sb, a.noise[at * 3 + d]));
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a.pos_next[at * 3 + d] = xn[d];
        if (a.pos_cur) a.pos_cur[at * 3 + d] = xn[d];
    }
    // ---- types (:682-685)
    float lg[TD_MAXC];
    float mx = -INFINITY;
#pragma unroll
    for (int cc = 0; cc < TD_MAXC; ++cc) {
        lg[cc] = cc < C ? a.pred_v[at * C + cc] : -INFINITY;
        mx = fmaxf(mx, lg[cc]);
    }
    float se = 0.f;
#pragma unroll
    for (int cc = 0; cc < TD_MAXC; ++cc) se += cc < C ? expf(lg[cc] - mx) : 0.f;
    const float lse = mx + logf(se);
    const int tm1 = t - 1 < 0 ? 0 : t - 1;
    const float lnK = logf((float)C);
    const float l_ca = PROG ? prow[TD_PROG_LOG_CA] : sc.log_ca[tm1], l_1mca = (PROG ? prow[TD_PROG_LOG_1MCA] : sc.log_1mca[tm1]) - lnK;
    const float l_a = PROG ? prow[TD_PROG_LOG_A] : sc.log_a[t], l_1ma = (PROG ? prow[TD_PROG_LOG_1MA] : sc.log_1ma[t]) - lnK;
    const float LOG_EPS = logf(1e-30f);                         // log(clamp(onehot, 1e-30)), :129
    float un[TD_MAXC];
    float umx = -INFINITY;
#pragma unroll
    for (int cc = 0; cc < TD_MAXC; ++cc) {
        if (cc < C) {
            const float lv0 = lg[cc] - lse;                     // log_softmax
            lg[cc] = lv0;
            const float lvt = cc == vt ? 0.f : LOG_EPS;
            un[cc] = td_log_add_exp(lv0 + l_ca, l_1mca) + td_log_add_exp(lvt + l_a, l_1ma);
            umx = fmaxf(umx, un[cc]);
        } else {
            un[cc] = -INFINITY;
        }
    }
    float us = 0.f;
#pragma unroll
    for (int cc = 0; cc < TD_MAXC; ++cc) us += cc < C ? expf(un[cc] - umx) : 0.f;
    const float ulse = umx + logf(us);
    const int v0k = FIXED && known ? (int)a.fixed_v[at] : 0;
    int best = 0;
    float bestv = -INFINITY;
#pragma unroll
    for (int cc = 0; cc < TD_MAXC; ++cc) {
        if (cc < C) {
            float lp = un[cc] - ulse;
            if (FIXED && known)         // q(v_{t-1} | v0) (:383-392) at level t - 1; t == 0: the known type itself
                lp = last ? (cc == v0k ? 0.f : LOG_EPS) : td_log_add_exp((cc == v0k ? 0.f : LOG_EPS) + l_ca, l_1mca);
            if (a.log_v0) a.log_v0[at * C + cc] = lg[cc];
            if (a.log_post) a.log_post[at * C + cc] = lp;
            const float gum = td_gumbel(a.uni[at * C + cc]);
            const float sc2 = gum + lp;
            if (sc2 > bestv) { bestv = sc2; best = cc; }        // first maximum, like argmax
        }
    }
    if (FIXED && known && last) best = v0k;
    if (a.v_frozen) best = vt;
    a.v_next[at] = best;
    if (a.v_cur) a.v_cur[at] = best;
}

template <bool FIXED, bool PROG, bool GUIDED>
__global__ void posterior_kernel(TdSchedules sc, TdStepArgs a) {
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= a.Nl) return;
    a.pos_cur = nullptr, a.v_cur = nullptr, a.v_frozen = false;      // the stateless form has none of them: known at compile time
    td_posterior_atom<FIXED, PROG, GUIDED>(sc, a, at);
}

// the last workgroup to finish advances the step index (all workgroups have read it by then): the launch is replayable as a graph node
__device__ __forceinline__ void td_step_handover(int32_t *__restrict__ step) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(step + 1, 1) == (int)gridDim.x - 1) {
            step[1] = 0;
            atomicAdd(step, 1);
        }
    }
}

// td_session_step: the same update with its per-step arguments taken from device memory -- step index s = step[0] selects the
// time-step row t_all[s] and slot s of the trajectories (and row s of a program's coefficient table); the current state (pos / v,
// which the caller also names as pos_cur / v_cur) is updated in place.
__device__ __forceinline__ void td_step_resolve(TdStepArgs &a, const TdStepSlot &sl) {
    int s = *reinterpret_cast<volatile int32_t *>(sl.step);
    s = s < 0 ? 0 : (s >= sl.num_steps ? sl.num_steps - 1 : s);
    const size_t so = (size_t)s * (size_t)a.Nl;
    a.t = sl.t_all + (size_t)s * a.B;
    a.pos_next = sl.pos_traj + so * 3;
    a.v_next = sl.v_traj + so;
    a.log_v0 = sl.v0_traj ? sl.v0_traj + so * a.C : nullptr;
    a.log_post = sl.vt_traj ? sl.vt_traj + so * a.C : nullptr;
    a.prow = sl.prog_table ? sl.prog_table + (size_t)s * TD_PROG_ROW : nullptr;
    if (sl.pos_only) {
        a.v_cur = nullptr;
        a.v_frozen = true;
    }
}

template <bool FIXED, bool PROG, bool GUIDED>
__global__ void posterior_step_kernel(TdSchedules sc, TdStepArgs a, TdStepSlot sl) {
    td_step_resolve(a, sl);
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at < a.Nl) td_posterior_atom<FIXED, PROG, GUIDED>(sc, a, at);
    td_step_handover(sl.step);
}

// ------------------------------------------------------------------------------------------ renoise (time programs)
// One ligand atom of a forward-process step s -> t over any number of levels: every atom alike, known ones too.
//   x' = sqrt(rho) x + sqrt(1 - rho) eps, rho = abar[t] / abar[s]  (roots in fp32, the products and the sum each rounded on their own)
//   log q(v_t = c | v_s) = log_add_exp(log(clamp(onehot(v_s), 1e-30))_c + l_r, log1m(l_r) - ln K), v' = argmax_c(gumbel(u_c) + log q_c)
// Reads a.prow (the slot's row), C, pos, v, noise, uni and writes pos_next, v_next, log_v0 (the log one-hot of v_s), log_post (log q)
// and the second copies.  uni == nullptr (pos_only): the types are not touched.  pos / v may alias pos_next / v_next.
__device__ __forceinline__ void td_renoise_atom(const TdStepArgs &a, int64_t at) {
    const int C = a.C;
    const float rho = a.prow[TD_PROG_RHO];
    const float sa = sqrtf(rho), sb = sqrtf(1.0f - rho);
    float xn[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) xn[d] = td_add_rn(td_mul_rn(sa, a.pos[at * 3 + d]), td_mul_rn(sb, a.noise[at * 3 + d]));
    const int vs = (int)a.v[at];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a.pos_next[at * 3 + d] = xn[d];
        if (a.pos_cur) a.pos_cur[at * 3 + d] = xn[d];
    }
    int best = vs;
    if (a.uni) {
        const float l_r = a.prow[TD_PROG_LOG_R], l_1mr = a.prow[TD_PROG_LOG_1MR] - logf((float)C);
        const float LOG_EPS = logf(1e-30f);
        float bestv = -INFINITY;
        best = 0;
        for (int cc = 0; cc < C; ++cc) {
            const float l0 = cc == vs ? 0.f : LOG_EPS;
            const float lq = td_log_add_exp(l0 + l_r, l_1mr);
            if (a.log_v0) a.log_v0[at * C + cc] = l0;
            if (a.log_post) a.log_post[at * C + cc] = lq;
            const float gum = td_gumbel(a.uni[at * C + cc]);
            const float sc2 = gum + lq;
            if (sc2 > bestv) { bestv = sc2; best = cc; }        // first maximum, like argmax
        }
    }
    a.v_next[at] = best;
    if (a.v_cur) a.v_cur[at] = best;
}

__global__ void renoise_kernel(TdStepArgs a) {
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= a.Nl) return;
    a.pos_cur = nullptr, a.v_cur = nullptr;
    td_renoise_atom(a, at);
}

// the session-step form: slot s = step[0] of the trajectories and row s of the table, the state in place, the step index advanced
__global__ void renoise_step_kernel(TdStepArgs a, TdStepSlot sl) {
    td_step_resolve(a, sl);
    if (sl.pos_only) a.uni = nullptr;
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at < a.Nl) td_renoise_atom(a, at);
    td_step_handover(sl.step);
}

// a workgroup of 128 atoms
static dim3 step_grid(const TdStepArgs &a) { return dim3((unsigned)((a.Nl + 127) / 128)); }

// known atoms present: the variant with the replacement branch (needs sc.abar, checked by the callers); a program slot: the variant
// that reads the slot's row; a shift of x0 (clash guidance): the variant that adds it
int td_launch_posterior(const TdSchedules &sc, const TdStepArgs &a, hipStream_t s) {
    if (a.Nl == 0) return TD_OK;
    td_dispatch3(a.fixed_mask != nullptr, a.prow != nullptr, a.x0_shift != nullptr, [&](auto F, auto P, auto G) {
        posterior_kernel<F.value, P.value, G.value><<<step_grid(a), dim3(128), 0, s>>>(sc, a);
    });
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_posterior_step(const TdSchedules &sc, const TdStepArgs &a, const TdStepSlot &sl, hipStream_t s) {
    if (a.Nl == 0) return TD_OK;
    td_dispatch3(a.fixed_mask != nullptr, sl.prog_table != nullptr, a.x0_shift != nullptr, [&](auto F, auto P, auto G) {
        posterior_step_kernel<F.value, P.value, G.value><<<step_grid(a), dim3(128), 0, s>>>(sc, a, sl);
    });
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_renoise(const TdStepArgs &a, hipStream_t s) {
    if (a.Nl == 0) return TD_OK;
    renoise_kernel<<<step_grid(a), dim3(128), 0, s>>>(a);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

int td_launch_renoise_step(const TdStepArgs &a, const TdStepSlot &sl, hipStream_t s) {
    if (a.Nl == 0) return TD_OK;
    renoise_step_kernel<<<step_grid(a), dim3(128), 0, s>>>(a, sl);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

// ------------------------------------------------------------------------------------------ centring
__global__ __launch_bounds__(256) void center_kernel(float *__restrict__ ppos, const int32_t *__restrict__ pptr,
                                                     float *__restrict__ lpos, const int32_t *__restrict__ lptr,
                                                     float *__restrict__ offset, int compute, float sign) {
    __shared__ float s_off[3];
    const int g = blockIdx.x;
    if (compute) {
        // scatter_mean (models/molopt_score_model.py:115): sum / clamp(count, 1).  The sum runs over the graph's atoms IN INDEX
        // ORDER, one thread per coordinate -- the order of the reference's CPU path (index_add_ walks the rows sequentially), so
        // the centred coordinates, and with them every near-tie of the k-NN search, come out bit-identical to it.  (A tree
        // reduction differs in the last bit of the offset: one neighbour flip in 1000 teacher-forced steps on 1h36, round 3.)
        if (threadIdx.x < 3) {
            const int b = pptr[g], e = pptr[g + 1];
            float sum = 0.f;
            for (int i = b; i < e; ++i) sum += ppos[3 * i + threadIdx.x];
            const int cnt = e - b;
            const float o = sum / (float)(cnt < 1 ? 1 : cnt);
            s_off[threadIdx.x] = o;
            offset[3 * g + threadIdx.x] = o;
        }
    } else if (threadIdx.x < 3) {
        s_off[threadIdx.x] = offset[3 * g + threadIdx.x];
    }
    __syncthreads();
    const float ox = sign * s_off[0], oy = sign * s_off[1], oz = sign * s_off[2];
    if (ppos) {
        for (int i = pptr[g] + threadIdx.x; i < pptr[g + 1]; i += blockDim.x) {
            ppos[3 * i] += ox; ppos[3 * i + 1] += oy; ppos[3 * i + 2] += oz;
        }
    }
    if (lpos) {
        for (int i = lptr[g] + threadIdx.x; i < lptr[g + 1]; i += blockDim.x) {
            lpos[3 * i] += ox; lpos[3 * i + 1] += oy; lpos[3 * i + 2] += oz;
        }
    }
}

int td_launch_center(float *ppos, const int32_t *pptr, float *lpos, const int32_t *lptr, int64_t B, float *offset,
                     int compute, int sign, hipStream_t s) {
    if (B == 0) return TD_OK;
    center_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(ppos, pptr, lpos, lptr, offset, compute,
                                                         sign < 0 ? -1.f : 1.f);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}

// ------------------------------------------------------------------------------------------ test hook
__global__ void reductions_kernel(const float *__restrict__ in, float *__restrict__ out) {
    const int l = threadIdx.x;
    const float v = in[l];
    out[0 * 64 + l] = td_sum8(v);
    out[1 * 64 + l] = td_sum32(v);
    out[2 * 64 + l] = td_sum64(v);
    out[3 * 64 + l] = td_sum_halves(v);
    out[4 * 64 + l] = td_max_halves(v);
    out[5 * 64 + l] = td_swap32(v);
}
int td_launch_reductions(const float *in, float *out, hipStream_t s) {
    reductions_kernel<<<dim3(1), dim3(64), 0, s>>>(in, out);
    TD_CHECK_HIP(hipGetLastError());
    return TD_OK;
}
