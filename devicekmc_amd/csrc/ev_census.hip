// ev_census.hip -- rate census of an event table (dkmc_event_rate_census; include/devicekmc_hip.h).  No counterpart in the reference.
//
// Which class carries the total rate, and how hot the sites that fire are, without copying N * nn doubles to the host.  A pure function of the
// caller's table: the class of a slot with P > 0 is recomputed from (element[i], element[j]) exactly as slot_rate does (events.hip), the deciding
// site s is j for generation and i for the three other classes.  Rows are read as k_ev_build reads them -- one wave per row, lanes striding the nn
// slots --, 12 B per slot (rate + neighbour) plus one element[j] gather per live slot.  No floating-point atomics: lane -> wave -> workgroup
// partials in a fixed order, then one single-workgroup fold (as k_current_info, current.hip); the grid depends on N only, so the same table gives
// the same bits on every call.
#include "common.h"

#define EVC_WORDS 16          // doubles of a workgroup partial: counts [0..3], sums [4..7], T-weighted sums [8..11], max, its slot, non-finite, 0
#define EVC_MAXBLOCKS 1024

// (P, slot) of the larger rate, the smaller slot among equal rates; slot < 0 = none yet
__device__ __forceinline__ void evc_take(double &P, long long &slot, double P2, long long slot2)
{
    if (slot2 >= 0 && (slot < 0 || P2 > P || (P2 == P && slot2 < slot))) { P = P2; slot = slot2; }
}

__global__ __launch_bounds__(256) void k_ev_census(int N, int nn, const int *__restrict__ neigh, const int *__restrict__ element,
                                                   const double *__restrict__ temperature, const double *__restrict__ ev_prob,
                                                   double *__restrict__ part)
{
    __shared__ double sh[4][EVC_WORDS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double cnt[4] = {0.0, 0.0, 0.0, 0.0}, sum[4] = {0.0, 0.0, 0.0, 0.0}, sumT[4] = {0.0, 0.0, 0.0, 0.0};
    double pmax = 0.0, nonfinite = 0.0; long long smax = -1;
    for (int i = blockIdx.x * 4 + w; i < N; i += gridDim.x * 4) {
        const int ei = element[i];
        const double T_i = temperature ? temperature[i] : 0.0;
        for (int c = lane; c < nn; c += WAVE) {
            const size_t idx = (size_t)i * nn + c;
            const double P = ev_prob[idx];
            if (!(P > 0.0)) { if (P != P) nonfinite += 1.0; continue; }       // zero (or negative) rate: nothing; NaN: non-finite
            if (isinf(P)) { nonfinite += 1.0; continue; }
            evc_take(pmax, smax, P, (long long)idx);
            const int j = neigh[idx];
            if (j < 0 || j >= N) continue;
            const int ej = element[j];
            const bool gen = (ei == DEFECT && ej == O_EL), rec = (ei == OXYGEN_DEFECT && ej == VACANCY);
            const bool vdf = (ei == VACANCY && ej == O_EL), idf = (ei == OXYGEN_DEFECT && ej == DEFECT);
            if (!(gen || rec || vdf || idf)) continue;
            const int cls = gen ? EV_GEN : rec ? EV_REC : vdf ? EV_VDIFF : EV_IDIFF;
            const double PT = temperature ? P * (gen ? temperature[j] : T_i) : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q == cls) { cnt[q] += 1.0; sum[q] += P; sumT[q] += PT; }
        }
    }
    // wave: the butterfly's fixed order; the (rate, slot) pair by a rule that does not depend on the order
#pragma unroll
    for (int q = 0; q < 4; ++q) { cnt[q] = wave_sum_all(cnt[q]); sum[q] = wave_sum_all(sum[q]); sumT[q] = wave_sum_all(sumT[q]); }
    nonfinite = wave_sum_all(nonfinite);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double P2 = __shfl_xor(pmax, off, WAVE);
        const long long s2 = __shfl_xor(smax, off, WAVE);
        evc_take(pmax, smax, P2, s2);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { sh[w][q] = cnt[q]; sh[w][4 + q] = sum[q]; sh[w][8 + q] = sumT[q]; }
        sh[w][12] = pmax; sh[w][13] = (double)smax; sh[w][14] = nonfinite; sh[w][15] = 0.0;
    }
    __syncthreads();
    // workgroup: waves 0, 1, 2, 3 in that order
    if (threadIdx.x < EVC_WORDS) {
        const int q = threadIdx.x;
        double v;
        if (q == 12 || q == 13) {
            double P = sh[0][12]; long long s = (long long)sh[0][13];
            for (int k = 1; k < 4; ++k) evc_take(P, s, sh[k][12], (long long)sh[k][13]);
            v = q == 12 ? P : (double)s;
        } else v = ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
        part[(size_t)blockIdx.x * EVC_WORDS + q] = v;
    }
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order, then the fixed-order block sum
__global__ __launch_bounds__(256) void k_ev_census_fold(int nb, const double *__restrict__ part, double *__restrict__ info)
{
    __shared__ double red[4], redP[256], redS[256];
    double acc[EVC_WORDS];
#pragma unroll
    for (int q = 0; q < EVC_WORDS; ++q) acc[q] = 0.0;
    double P = 0.0; long long s = -1;
    for (int b = threadIdx.x; b < nb; b += 256) {
        const double *p = part + (size_t)b * EVC_WORDS;
#pragma unroll
        for (int q = 0; q < EVC_WORDS; ++q) if (q != 12 && q != 13) acc[q] += p[q];
        evc_take(P, s, p[12], (long long)p[13]);
    }
#pragma unroll
    for (int q = 0; q < EVC_WORDS; ++q) if (q != 12 && q != 13) acc[q] = block_sum_all<256>(acc[q], red);
    redP[threadIdx.x] = P; redS[threadIdx.x] = (double)s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            double P1 = redP[threadIdx.x]; long long s1 = (long long)redS[threadIdx.x];
            evc_take(P1, s1, redP[threadIdx.x + h], (long long)redS[threadIdx.x + h]);
            redP[threadIdx.x] = P1; redS[threadIdx.x] = (double)s1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) info[q] = acc[q];
        info[12] = redS[0] >= 0.0 ? redP[0] : 0.0; info[13] = redS[0]; info[14] = acc[14];
        info[15] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    }
}

int ev_census_enqueue(int N, int nn, const int *neigh, const int *element, const double *temperature, const double *ev_prob, double **d_info16)
{
    hipStream_t st = eng().stream;
    const int nb = grid_blocks(N, 4, EVC_MAXBLOCKS);
    double *part = (double *)scratch(S_EV_CENSUS_PART, (size_t)EVC_MAXBLOCKS * EVC_WORDS * 8);
    double *info = (double *)scratch(S_EV_CENSUS_INFO, 16 * 8);
    if (!part || !info) return eng().err_code;
    hipLaunchKernelGGL(k_ev_census, dim3(nb), dim3(256), 0, st, N, nn, neigh, element, temperature, ev_prob, part);
    hipLaunchKernelGGL(k_ev_census_fold, dim3(1), dim3(256), 0, st, nb, (const double *)part, info);
    KCHK();
    *d_info16 = info;
    return 0;
}

extern "C" int dkmc_event_rate_census(int N, int nn, const int *d_neigh, const int *d_site_element, const double *d_site_temperature,
                                      const double *d_ev_prob, double *h_info16)
{
    if (N <= 0 || nn <= 0 || !d_neigh || !d_site_element || !d_ev_prob || !h_info16)
        return dkmc_fail(13, "event_rate_census: bad arguments", __FILE__, __LINE__);
    double *info = nullptr;
    if (ev_census_enqueue(N, nn, d_neigh, d_site_element, d_site_temperature, d_ev_prob, &info)) return eng().err_code;
    HIPCHK(hipMemcpyAsync(h_info16, info, 16 * 8, hipMemcpyDeviceToHost, eng().stream));
    HIPCHK(hipStreamSynchronize(eng().stream));
    return 0;
}
