// kernels_score.hip — log-probabilities of logit rows: per row log softmax at a target (SamplingUtils.cs:35-41), the ArgMax
// (SamplingUtils.cs:55-56: first index of the maximum) and its log-probability, over column slabs so that a [T][V] logit matrix
// never has to exist (nfai_hip_score_rows, nfai_hip_llama_score).
//
// A plain bandwidth kernel: every logit is read once, 16 bytes per lane where the row is 16-byte aligned.  One workgroup of 256
// threads per row; a thread walks its columns in increasing order with a running maximum (strict >: the first index stays) and
// four sums of exp(l - max) rescaled whenever its maximum moves; the threads meet by DPP inside the wave (wave_max / wave_sum /
// wave_best) and through 4 x 3 words of LDS across the waves, merged in wave order: deterministic for a given slab width.
#include <float.h>

#include "common.h"

namespace nfai {

// The running maximum starts at -FLT_MAX, not -inf: exp(l - m) is then 0, not NaN, for whatever comes first, and the first real
// logit replaces it (its sum is 0 * exp(-FLT_MAX - l) + 1).
struct ScoreLane {
    float m = -FLT_MAX;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    uint32_t idx = SCORE_NO_TARGET;
    __device__ __forceinline__ void raise(float nm)   // nm > m
    {
        const float f = __expf(m - nm);
        s *= f;
        m = nm;
    }
    __device__ __forceinline__ void one(float v, uint32_t j)
    {
        if (v > m) { raise(v); idx = j; }
        s[0] += __expf(v - m);
    }
    __device__ __forceinline__ void four(f32x4 v, uint32_t j)
    {
        const float vm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        if (vm > m) {
            raise(vm);
            idx = v[0] == vm ? j : (v[1] == vm ? j + 1 : (v[2] == vm ? j + 2 : j + 3));
        }
#pragma unroll
        for (int e = 0; e < 4; e++) s[e] += __expf(v[e] - m);
    }
};

__global__ __launch_bounds__(256) void k_score_slab(const float *slab, uint64_t ld, uint32_t c0, uint32_t ns, uint32_t V, const uint32_t *targets,
                                                    ScoreState *state, uint32_t *err)
{
    __shared__ float lds_m[4], lds_s[4];
    __shared__ uint32_t lds_i[4];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *p = slab + (uint64_t)row * ld;
    ScoreLane a;
    uint32_t done = 0;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {   // (wave-uniform) 16-byte loads over the multiple of 4; the tail below
        const uint32_t n4 = ns / 4;
        const f32x4 *p4 = reinterpret_cast<const f32x4 *>(p);
        for (uint32_t q = tid; q < n4; q += 256) a.four(p4[q], c0 + 4 * q);
        done = n4 * 4;
    }
    for (uint32_t j = done + tid; j < ns; j += 256) a.one(p[j], c0 + j);
    // the wave: its maximum, every lane's sums brought to it, the first index of it
    const float wm = wave_max(a.m);
    float s = ((a.s[0] + a.s[1]) + (a.s[2] + a.s[3])) * __expf(a.m - wm);
    s = wave_sum(s);
    float bv = a.m;
    uint32_t bi = a.idx;
    wave_best(bv, bi);
    if (lane == 0) { lds_m[wave] = wm; lds_s[wave] = s; lds_i[wave] = bi; }
    __syncthreads();
    if (tid != 0) return;
    ScoreState st;
    if (c0 == 0) {
        st.m = -FLT_MAX; st.s = 0.f; st.idx = SCORE_NO_TARGET; st.tl = 0.f;
    } else {
        st = state[row];
    }
    for (int w = 0; w < 4; w++) {   // the sums in wave order; among equal maxima the lower index (the waves' columns interleave)
        const float om = lds_m[w], os = lds_s[w];
        if (om > st.m) {
            st.s = st.s * __expf(st.m - om) + os;
            st.m = om;
            st.idx = lds_i[w];
        } else {
            st.s += os * __expf(om - st.m);
            if (om == st.m && lds_i[w] < st.idx) st.idx = lds_i[w];
        }
    }
    const uint32_t t = targets[row];
    if (t != SCORE_NO_TARGET) {
        if (t >= V) {
            if (c0 == 0) atomicOr(err, 1u);
        } else if (t >= c0 && t - c0 < ns) {
            st.tl = p[t - c0];
        }
    }
    state[row] = st;
}

__global__ __launch_bounds__(256) void k_score_finish(const ScoreState *state, uint32_t T, const uint32_t *targets, const uint32_t *err, float *logprob,
                                                      uint32_t *argmax, float *logprob_max)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= T || *err != 0) return;
    const ScoreState st = state[r];
    const float ls = logf(st.s);
    logprob[r] = targets[r] == SCORE_NO_TARGET ? 0.f : (st.tl - st.m) - ls;
    argmax[r] = st.idx;
    logprob_max[r] = -ls;
}

hipError_t launch_score_slab(const float *slab, uint32_t T, uint64_t ld, uint32_t c0, uint32_t ns, uint32_t V, const uint32_t *targets, ScoreState *state,
                             uint32_t *err, hipStream_t s)
{
    if (!slab || !targets || !state || !err || T == 0 || ns == 0 || ld < ns || c0 >= V || ns > V - c0) return hipErrorInvalidValue;
    k_score_slab<<<T, 256, 0, s>>>(slab, ld, c0, ns, V, targets, state, err);
    return hipGetLastError();
}

hipError_t launch_score_finish(const ScoreState *state, uint32_t T, const uint32_t *targets, const uint32_t *err, float *logprob, uint32_t *argmax,
                               float *logprob_max, hipStream_t s)
{
    if (!state || !targets || !err || !logprob || !argmax || !logprob_max || T == 0) return hipErrorInvalidValue;
    k_score_finish<<<(T + 255) / 256, 256, 0, s>>>(state, T, targets, err, logprob, argmax, logprob_max);
    return hipGetLastError();
}

}  // namespace nfai
