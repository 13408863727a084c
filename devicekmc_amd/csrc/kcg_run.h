// kcg_run.h -- the loop of the K-CG (kcg.hip) without K's assembly: what a caller that brings its own stored words, diagonal and right-hand side needs.
// K itself (kcg_assemble_and_solve) and the local heat model (heat.hip, dkmc_set_heat_form) run on it.  Host code only; every kernel is kcg.hip's.
#pragma once
#include "common.h"

struct KCtrl { double rr[2]; double pad; int done; int iters; };

// One system on one of the three forms.  rp / nnz: the CSR positions (kb null); kb: a blocked form (form 1 or 2) of the same pattern.
// cf: the stored words in the form's layout (CSR: one int per position; blocked: kb->total words of kb->word_bytes bytes); diag, rhs: in the form's
// row order (rhs is scaled in place); y_site: start vector in, solution out, in the pattern's row order; yb: m doubles of work space, blocked forms only.
struct KcgRun {
    int m = 0, nnz = 0;
    const int *rp = nullptr; const KBlocked *kb = nullptr; const int *cf = nullptr; const double *diag = nullptr;
    double *rhs = nullptr, *y_site = nullptr, *y = nullptr;
    double w_high = 0.0, w_low = 0.0, tol2 = 0.0;
    double *s = nullptr, *r = nullptr, *p = nullptr, *t = nullptr, *q = nullptr, *part = nullptr;
    KCtrl *ctrl = nullptr;          // the stop word the iteration kernels read
    bool kbw = false, kbw2 = false;
    int ga = 0, gv = 0, npa = 0, vb = 0; size_t lds = 0;
    int syncs = 0;                  // host synchronisations of kcg_run_poll so far
    double ms = 0.0; int iters_timed = 0;       // profiling on: HIP-event time of the polled loop
};
int kcg_run_setup(KcgRun &c, int m, const int *rp, int nnz, const KBlocked *kb, const int *cf, const double *diag, double *rhs, double *yb,
                  double w_high, double w_low, double tol, double *y_site);
// scale + the two memsets; start product, q, first stop test.  ctrl_out: where the start leaves the stop word (c.ctrl, or a copy the caller arms itself)
int kcg_run_scale(KcgRun &c, KCtrl *ctrl_out);
int kcg_run_start(KcgRun &c, KCtrl *ctrl_out);
int kcg_run_iterate(KcgRun &c, int it);                 // the launches of iteration `it`; they return at once when c.ctrl->done is set
int kcg_run_poll(KcgRun &c, KCtrl &h, int first);       // the host's poll loop; first > 0: that many iterations are enqueued before the first poll
int kcg_run_unscale(KcgRun &c);
long long kcg_run_bytes(const KcgRun &c);               // bytes one iteration moves
// all of it: scale, start, poll, unscale
int kcg_run(KcgRun &c, KCtrl &h, int first);
