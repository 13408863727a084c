// split.hip -- solve_sparse_CG_splitmatrix (iterative_solvers_gpu.cu:656-821) + add_submatrix_product (:634-652).
//
// The reference's split path keeps the current-solve matrix as a sparse neighbour part A (CSR, m rows) plus a dense tunnel block M
// (msub x msub, row-major) that couples the rows insertion_indices[k] + offset, and solves (A + P^T M P) y = x with an
// UNPRECONDITIONED CG: r = (A + M) y - x, p = -r, loop while ||r||_2 > tol (tol = 1e-5 in the source).  It is unfinished there: the
// function prints the solution and calls exit(1), and its caller update_power_gpu_split is never reached (current_solver.cpp:21).
// This file completes the entry point with the same contract.  The product's own current solve does not come through here: it
// keeps M as symmetric tiles of its upper triangle (xt.hip), which is this idea at 4.5 B per entry instead of 8 B and without the
// zeros of the dense block.
//
// add_submatrix_product in the reference: one THREAD per row of M walking msub columns (uncoalesced, one wave touches 64 rows).
// Here: one workgroup per 32 rows of M; the gathered sub-vector p[idx] is staged through LDS in chunks of 1024 columns, every
// wave streams 8 rows with 16-byte loads, row sums are combined in a fixed order; each row of M is summed by exactly one
// workgroup, so the result is added to t without atomics.  HBM-bound: 8 B per entry of M per iteration.
#include "cg_host.h"

#define SP_NT 256
struct SCtrl { double rr; double pad; int done; int iters; };
typedef double dbl2 __attribute__((ext_vector_type(2)));

// t = A p (CSR, 8 lanes per row): blocks [0, nab).  t_sub = M p_sub for 32 rows of M per block: blocks [nab, nab + nmb); written to
// tsub[row of M] (added to t by the step kernels through idx).
__global__ __launch_bounds__(SP_NT) void k_sp_apply(int m, const int *__restrict__ rp, const int *__restrict__ ci, const double *__restrict__ a,
                                                    const double *__restrict__ p, double *__restrict__ t, int nab,
                                                    int msub, const double *__restrict__ M, const int *__restrict__ idx, int off,
                                                    double *__restrict__ tsub, const SCtrl *ctrl)
{
    __shared__ double pv[1024];
    __shared__ double part[SP_NT / 64][8];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    __syncthreads();
    if (sdone) return;
    if ((int)blockIdx.x < nab) {
        const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
        for (int row = blockIdx.x * (SP_NT / 8) + g; row < m; row += nab * (SP_NT / 8)) {
            const int p0 = rp[row], p1 = rp[row + 1];
            double s = 0.0;
            for (int q = p0 + l; q < p1; q += 8) s += a[q] * p[ci[q]];
            s = group_sum<8>(s);
            if (l == 0) t[row] = s;
        }
        return;
    }
    // dense block: rows r0 .. r0 + 31 of M; wave w takes rows r0 + 8 w .. + 7, lane handles column pairs
    const int r0 = ((int)blockIdx.x - nab) * 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    for (int c0 = 0; c0 < msub; c0 += 1024) {
        const int nc = min(1024, msub - c0);
        __syncthreads();
        for (int c = threadIdx.x; c < 1024; c += SP_NT) pv[c] = c < nc ? p[idx[c0 + c] + off] : 0.0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = r0 + 8 * w + j;
            if (row >= msub) continue;
            const double *mr = M + (size_t)row * msub + c0;
            double s = 0.0;
            if ((((size_t)row * msub + c0) & 1) == 0) {                  // 16-byte aligned row segment
                for (int c = 2 * lane; c + 1 < nc; c += 128) { const dbl2 v = *reinterpret_cast<const dbl2 *>(mr + c); s += v.x * pv[c] + v.y * pv[c + 1]; }
                if ((nc & 1) && lane == 0) s += mr[nc - 1] * pv[nc - 1];
            } else {
                for (int c = lane; c < nc; c += 64) s += mr[c] * pv[c];
            }
            acc[j] += s;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double s = wave_sum(acc[j]);
        if (lane == 0) part[w][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < 32) { const int row = r0 + (int)threadIdx.x; if (row < msub) tsub[row] = part[threadIdx.x >> 3][threadIdx.x & 7]; }
}

// t[idx[k] + off] += tsub[k]   (insertion_indices are distinct)
__global__ void k_sp_scatter(int msub, const int *__restrict__ idx, int off, const double *__restrict__ tsub, double *__restrict__ t, const SCtrl *ctrl)
{
    if (ctrl && ctrl->done) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < msub) t[idx[k] + off] += tsub[k];
}
// r = t - x ; p = -r ; partial r.r
__global__ __launch_bounds__(SP_NT) void k_sp_init(int m, const double *__restrict__ t, const double *__restrict__ x, double *__restrict__ r,
                                                   double *__restrict__ p, double *__restrict__ part)
{
    __shared__ double red[SP_NT / 64];
    double acc = 0.0;
    for (int i = blockIdx.x * SP_NT + threadIdx.x; i < m; i += gridDim.x * SP_NT) { const double rv = t[i] - x[i]; r[i] = rv; p[i] = -rv; acc += rv * rv; }
    const double tot = block_sum_all<SP_NT>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ __launch_bounds__(SP_NT) void k_sp_check(const double *part, int n, SCtrl *ctrl, double tol, int it)
{
    __shared__ double red[SP_NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += SP_NT) s += part[i];
    const double rr = block_sum_all<SP_NT>(s, red);
    if (threadIdx.x == 0) { ctrl->rr = rr; ctrl->iters = it; ctrl->done = !(sqrt(rr) > tol); }      // while (h_norm > tol), :757
}
// partial p.t
__global__ __launch_bounds__(SP_NT) void k_sp_dot(int m, const double *__restrict__ p, const double *__restrict__ t, double *__restrict__ part, const SCtrl *ctrl)
{
    __shared__ double red[SP_NT / 64];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    __syncthreads();
    if (sdone) return;
    double acc = 0.0;
    for (int i = blockIdx.x * SP_NT + threadIdx.x; i < m; i += gridDim.x * SP_NT) acc += p[i] * t[i];
    const double tot = block_sum_all<SP_NT>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// alpha = r.r / p.t ; y += alpha p ; r += alpha t ; partial r'.r'
__global__ __launch_bounds__(SP_NT) void k_sp_update(int m, const double *__restrict__ part_pt, int n, const double *__restrict__ p,
                                                     const double *__restrict__ t, double *__restrict__ y, double *__restrict__ r,
                                                     double *__restrict__ part_rr, const SCtrl *ctrl)
{
    __shared__ double red[SP_NT / 64];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += SP_NT) s += part_pt[i];
    const double pAp = block_sum_all<SP_NT>(s, red);
    if (sdone) return;
    const double alpha = ctrl->rr / pAp;
    double acc = 0.0;
    for (int i = blockIdx.x * SP_NT + threadIdx.x; i < m; i += gridDim.x * SP_NT) {
        y[i] += alpha * p[i];
        const double rn = r[i] + alpha * t[i];
        r[i] = rn; acc += rn * rn;
    }
    const double tot = block_sum_all<SP_NT>(acc, red);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = tot;
}
// beta = r'.r' / r.r ; p = beta p - r' ; stop test on ||r'||
__global__ __launch_bounds__(SP_NT) void k_sp_direction(int m, int it, const double *__restrict__ part_rr, int n, const double *__restrict__ r,
                                                        double *__restrict__ p, SCtrl *ctrl, double tol)
{
    __shared__ double red[SP_NT / 64];
    __shared__ int sdone;
    if (threadIdx.x == 0) sdone = ctrl->done;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += SP_NT) s += part_rr[i];
    const double rr_new = block_sum_all<SP_NT>(s, red);
    if (sdone) return;
    const double beta = rr_new / ctrl->rr;
    for (int i = blockIdx.x * SP_NT + threadIdx.x; i < m; i += gridDim.x * SP_NT) p[i] = p[i] * beta - r[i];
    (void)it; (void)tol;      // r.r of the next iteration is published by a follow-up launch (k_sp_publish): every block here has read the old one
}
__global__ void k_sp_publish(const double *part_rr, int n, SCtrl *ctrl, double tol, int it)
{
    __shared__ double red[SP_NT / 64];
    if (ctrl->done) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += SP_NT) s += part_rr[i];
    const double rr = block_sum_all<SP_NT>(s, red);
    if (threadIdx.x == 0) { ctrl->rr = rr; ctrl->iters = it + 1; if (!(sqrt(rr) > tol)) ctrl->done = 1; }
}

// A (CSR, m rows, int32) and M (msub x msub dense, row-major) are read only; x: right-hand side; y: start vector in, solution out.
// index_offset: the reference adds 2 to every insertion index (node = atom + 2, :646); pass 0 for plain row indices.
extern "C" int dkmc_solve_sparse_CG_splitmatrix(const double *M, int msub, const double *A_data, const int *A_row_ptr, const int *A_col_indices,
                                                int A_nnz, int m, const int *insertion_indices, int index_offset, const double *x, double *y,
                                                double tol, int *iters_out, double *rnorm_out)
{
    (void)A_nnz;
    Engine &e = eng(); hipStream_t st = e.stream;
    if (m <= 0) { if (iters_out) *iters_out = 0; if (rnorm_out) *rnorm_out = 0.0; return 0; }
    if (msub < 0 || (msub > 0 && (!M || !insertion_indices))) return dkmc_fail(14, "solve_sparse_CG_splitmatrix: bad dense block", __FILE__, __LINE__);
    double *r = (double *)scratch(S_CG_R, (size_t)m * 8), *p = (double *)scratch(S_CG_P, (size_t)m * 8), *t = (double *)scratch(S_CG_T, (size_t)m * 8);
    double *tsub = (double *)scratch(S_CG_PS, (size_t)(msub + 2) * 8);
    double *part = (double *)scratch(S_CG_PART, (size_t)3 * 8192 * 8);
    SCtrl *ctrl = (SCtrl *)scratch(S_CG_CTRL, 64);
    if (!r || !p || !t || !tsub || !part || !ctrl) return e.err_code;
    double *part_pt = part, *part_rr = part + 4096;
    const int nab = grid_blocks(m, SP_NT / 8, 4096), nmb = (msub + 31) / 32, gv = grid_blocks(m, SP_NT * 4, 512);
    HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(SCtrl), st));
    auto matvec = [&](const double *v) {
        hipLaunchKernelGGL(k_sp_apply, dim3(nab + nmb), dim3(SP_NT), 0, st, m, A_row_ptr, A_col_indices, A_data, v, t, nab, msub, M, insertion_indices,
                           index_offset, tsub, (const SCtrl *)ctrl);
        if (msub > 0) hipLaunchKernelGGL(k_sp_scatter, dim3((msub + 255) / 256), dim3(256), 0, st, msub, insertion_indices, index_offset, (const double *)tsub, t, (const SCtrl *)ctrl);
    };
    matvec(y);                                                                   // r = (A + M) y - x ; p = -r   (:729-745)
    hipLaunchKernelGGL(k_sp_init, dim3(gv), dim3(SP_NT), 0, st, m, (const double *)t, x, r, p, part_rr);
    hipLaunchKernelGGL(k_sp_check, dim3(1), dim3(SP_NT), 0, st, (const double *)part_rr, gv, ctrl, tol, 0);
    KCHK();
    SCtrl h{};
    if (int rc = cg_poll_loop(ctrl, h, LaunchPlan::doubling(8), st, "CG: no convergence after 200000 iterations", nullptr, [&](int it, const hipEvent_t *) -> int {
            matvec(p);
            hipLaunchKernelGGL(k_sp_dot, dim3(gv), dim3(SP_NT), 0, st, m, (const double *)p, (const double *)t, part_pt, (const SCtrl *)ctrl);
            hipLaunchKernelGGL(k_sp_update, dim3(gv), dim3(SP_NT), 0, st, m, (const double *)part_pt, gv, (const double *)p, (const double *)t, y, r, part_rr, (const SCtrl *)ctrl);
            hipLaunchKernelGGL(k_sp_direction, dim3(gv), dim3(SP_NT), 0, st, m, it, (const double *)part_rr, gv, (const double *)r, p, ctrl, tol);
            hipLaunchKernelGGL(k_sp_publish, dim3(1), dim3(SP_NT), 0, st, (const double *)part_rr, gv, ctrl, tol, it);
            return 0;
        })) return rc;
    if (iters_out) *iters_out = h.iters;
    if (rnorm_out) *rnorm_out = sqrt(h.rr);
    return e.err_code;
}
