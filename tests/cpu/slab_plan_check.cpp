// Stand-alone check of csrc/slab_plan.h (tests/test_slab_plan.py compiles it with -fsanitize=address,undefined and reads its output).
//   slab_plan_check plan <nr> <rows> <marked> <nr * (nr + 2) ints: nown | nmark | hal[s * nr + d]>
// prints rowoff, markoff, maxown, covers(rows, marked), and for every rank v its hsoff, hroff and its two halo lists: buffers of EXACTLY hsoff[nr] and
// hroff[nr] ints, pre-filled with -1, in which piece d (s) is written through the offsets as hal(v, d) (hal(s, v)) copies of d (s) -- an offset
// that is off ends in an AddressSanitizer report or shows as a gap (-1) or a wrong order in the printed buffer.
//   slab_plan_check a2a <nr> <nr * nr counts: cnt[a * nr + d]>
// the same for an all-to-all-v: for every rank r "send r" = its send buffer of exactly slab_send_off(r, nr) words with piece r -> d filled with d,
// "recv r" = its receive buffer of exactly slab_recv_off(nr, r) words with piece a -> r filled with a; then recvmax.
#include "slab_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void print(const char *name, int r, const int *v, size_t n)
{
    if (r >= 0) printf("%s%d", name, r); else printf("%s", name);
    for (size_t i = 0; i < n; ++i) printf(" %d", v[i]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "plan")) {
        const int nr = atoi(argv[2]);
        if (nr < 1 || nr > XS_MAXR || argc != 5 + (int)slab_tab_ints(nr)) { fprintf(stderr, "usage: see the head of slab_plan_check.cpp\n"); return 2; }
        std::vector<int> tab(slab_tab_ints(nr));
        for (size_t i = 0; i < tab.size(); ++i) tab[i] = atoi(argv[5 + i]);
        const SlabPlan P(tab.data(), nr);
        print("rowoff", -1, P.rowoff, (size_t)nr + 1); print("markoff", -1, P.markoff, (size_t)nr + 1);
        printf("maxown %d\ncovers %d\n", P.maxown, P.covers(atoi(argv[3]), atoi(argv[4])) ? 1 : 0);
        for (int v = 0; v < nr; ++v) {
            const SlabHalo H(P, v);
            print("hsoff", v, H.hsoff, (size_t)nr + 1); print("hroff", v, H.hroff, (size_t)nr + 1);
            int *hs = new int[H.hsoff[nr]], *hr = new int[H.hroff[nr]];
            for (int i = 0; i < H.hsoff[nr]; ++i) hs[i] = -1;
            for (int i = 0; i < H.hroff[nr]; ++i) hr[i] = -1;
            for (int d = 0; d < nr; ++d) {
                if (d == v) continue;
                for (int i = 0; i < P.hal(v, d); ++i) hs[H.hsoff[d] + i] = d;
                for (int i = 0; i < P.hal(d, v); ++i) hr[H.hroff[d] + i] = d;
            }
            print("hsend", v, hs, (size_t)H.hsoff[nr]); print("hrecv", v, hr, (size_t)H.hroff[nr]);
            delete[] hs; delete[] hr;
        }
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "a2a")) {
        const int nr = atoi(argv[2]);
        if (nr < 1 || nr > XS_MAXR || argc != 3 + nr * nr) { fprintf(stderr, "usage: see the head of slab_plan_check.cpp\n"); return 2; }
        std::vector<long long> cnt((size_t)nr * nr);
        for (size_t i = 0; i < cnt.size(); ++i) cnt[i] = atoll(argv[3 + i]);
        for (int r = 0; r < nr; ++r) {
            const long long ns = slab_send_off(cnt.data(), nr, r, nr), nv = slab_recv_off(cnt.data(), nr, nr, r);
            int *sb = new int[ns], *rb = new int[nv];
            for (long long i = 0; i < ns; ++i) sb[i] = -1;
            for (long long i = 0; i < nv; ++i) rb[i] = -1;
            for (int o = 0; o < nr; ++o) {
                for (long long i = 0; i < cnt[(size_t)r * nr + o]; ++i) sb[slab_send_off(cnt.data(), nr, r, o) + i] = o;
                for (long long i = 0; i < cnt[(size_t)o * nr + r]; ++i) rb[slab_recv_off(cnt.data(), nr, o, r) + i] = o;
            }
            print("send", r, sb, (size_t)ns); print("recv", r, rb, (size_t)nv);
            delete[] sb; delete[] rb;
        }
        printf("recvmax %lld\n", slab_recv_max(cnt.data(), nr));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "layout")) {
        int *itab = new int[slab_tab_bytes() / sizeof(int)];
        for (int i = 0; i < XS_BINS; ++i) itab[i] = 1;
        for (int i = 0; i < XS_MAXR + 2; ++i) itab[XS_CUTS_AT + i] = 2;
        for (size_t i = 0; i < slab_tab_ints(XS_MAXR); ++i) itab[XS_TAB_AT + i] = 3;
        long long sum = 0;
        for (size_t i = 0; i < slab_tab_bytes() / sizeof(int); ++i) sum += itab[i];
        printf("bytes %zu\nsum %lld\n", slab_tab_bytes(), sum);
        delete[] itab;
        return 0;
    }
    fprintf(stderr, "usage: see the head of slab_plan_check.cpp\n");
    return 2;
}
