// The per-atom atom-type term of compute_v_Lt (models/molopt_score_model.py:476-483), shared by likelihood_terms_kernel (likelihood.hip)
// and diffusion_loss_kernel (loss.hip): one body, so that for the same inputs both kernels hold the same bits.
#pragma once

#include "td_device.h"
#include "td_internal.h"

// q(v_{t-1} | v_t, v_0) in log space (:401-409) for one atom; log_v0 / out: [C] registers
__device__ __forceinline__ void td_q_v_posterior(const TdSchedules &sc, int t, int C, const float (&log_v0)[TD_MAXC], int vt,
                                                 float (&out)[TD_MAXC]) {
    const int tm1 = t - 1 < 0 ? 0 : t - 1;
    const float lnK = logf((float)C);
    const float l_ca = sc.log_ca[tm1], l_1mca = sc.log_1mca[tm1] - lnK;
    const float l_a = sc.log_a[t], l_1ma = sc.log_1ma[t] - lnK;
    const float LOG_EPS = logf(1e-30f);
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < TD_MAXC; ++c) {
        if (c < C) {
            const float lvt = c == vt ? 0.f : LOG_EPS;
            out[c] = td_log_add_exp(log_v0[c] + l_ca, l_1mca) + td_log_add_exp(lvt + l_a, l_1ma);
            mx = fmaxf(mx, out[c]);
        } else {
            out[c] = -INFINITY;
        }
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < TD_MAXC; ++c) s += c < C ? expf(out[c] - mx) : 0.f;
    const float lse = mx + logf(s);
#pragma unroll
    for (int c = 0; c < TD_MAXC; ++c) out[c] -= lse;
}

// One atom's term of compute_v_Lt, added to `acc`: from its logits pred_v[at][0..C), its type v0[at] and its perturbed type vt[at],
// categorical_kl(true posterior, model posterior) for t > 0 and -log_categorical(log_v0, model posterior) at t == 0 (`decoder`).
// LOG_EPS: logf(1e-30f).  A macro, not a function, on purpose: expanded inside likelihood_terms_kernel it is, up to the names of its locals,
// the body that kernel had before the term was shared, so hipcc emits the instructions it emitted then and td_likelihood_terms keeps its
// bits (kl_pos included: wrapped into a function, inline or not, the same statements made the vectoriser pair the position block's
// multiplies and adds differently, and kl_pos moved in its last bits).  It is a sequence of statements, not an expression: use it as a
// statement of its own, once per scope.  Its locals carry the prefix tt_; two of them are results a caller may use afterwards:
// tt_ex[c] = exp(logit_c - max) (0 for c >= C) and tt_se, their sum -- softmax(pred_v)[c] = tt_ex[c] / tt_se.
#define TD_TYPE_TERM(acc, sc, t, C, decoder, LOG_EPS, pred_v, v0, vt, at)                                                   \
    float tt_lg[TD_MAXC], tt_lv0[TD_MAXC], tt_pm[TD_MAXC], tt_pt[TD_MAXC], tt_ex[TD_MAXC];                                  \
    float tt_mx = -INFINITY;                                                                                                \
    _Pragma("unroll") for (int c = 0; c < TD_MAXC; ++c) {                                                                   \
        tt_lg[c] = c < (C) ? (pred_v)[(int64_t)(at) * (C) + c] : -INFINITY;                                                 \
        tt_mx = fmaxf(tt_mx, tt_lg[c]);                                                                                     \
    }                                                                                                                       \
    float tt_se = 0.f;                                                                                                      \
    _Pragma("unroll") for (int c = 0; c < TD_MAXC; ++c) {                                                                   \
        tt_ex[c] = c < (C) ? expf(tt_lg[c] - tt_mx) : 0.f;                                                                  \
        tt_se += tt_ex[c];                                                                                                  \
    }                                                                                                                       \
    const float tt_lse = tt_mx + logf(tt_se);                                                                               \
    const int tt_a0 = (int)(v0)[at], tt_vt = (int)(vt)[at];                                                                 \
    _Pragma("unroll") for (int c = 0; c < TD_MAXC; ++c) {                                                                   \
        tt_lg[c] = tt_lg[c] - tt_lse;                    /* log_softmax(pred_v) */                                          \
        tt_lv0[c] = c == tt_a0 ? 0.f : (LOG_EPS);        /* index_to_log_onehot(v0) */                                      \
    }                                                                                                                       \
    td_q_v_posterior(sc, t, C, tt_lg, tt_vt, tt_pm);     /* model posterior */                                              \
    td_q_v_posterior(sc, t, C, tt_lv0, tt_vt, tt_pt);    /* true posterior */                                               \
    float tt_klv = 0.f, tt_nllv = 0.f;                                                                                      \
    _Pragma("unroll") for (int c = 0; c < TD_MAXC; ++c) {                                                                   \
        if (c < (C)) {                                                                                                      \
            tt_klv += expf(tt_pt[c]) * (tt_pt[c] - tt_pm[c]);    /* categorical_kl(true, model) */                          \
            tt_nllv += expf(tt_lv0[c]) * tt_pm[c];               /* log_categorical(log_v0, model) */                       \
        }                                                                                                                   \
    }                                                                                                                       \
    (acc) += (decoder) ? -tt_nllv : tt_klv
