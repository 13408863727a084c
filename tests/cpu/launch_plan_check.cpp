// Stand-alone check of csrc/launch_plan.h (tests/test_launch_plan.py compiles it with -fsanitize=address,undefined and reads its output).
//   launch_plan_check plan <policy> <hint> <iters>     the batches a solve that stops after <iters> iterations enqueues, its polls, and the
//                                                      iteration indices of the sampled launches that count
//   launch_plan_check polls <policy> <hint> <lo> <hi>  polls(iters) for iters = lo ... hi
// policy: doubling (hint = first batch), minus8, three_quarters
#include "launch_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static LaunchPlan plan_of(const char *policy, int hint)
{
    if (!strcmp(policy, "doubling")) return LaunchPlan::doubling(hint);
    if (!strcmp(policy, "minus8")) return LaunchPlan::hinted_minus8(hint);
    if (!strcmp(policy, "three_quarters")) return LaunchPlan::hinted_three_quarters(hint);
    fprintf(stderr, "unknown policy %s\n", policy);
    exit(2);
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "polls")) {
        const LaunchPlan plan = plan_of(argv[2], atoi(argv[3]));
        for (int iters = atoi(argv[4]); iters <= atoi(argv[5]); ++iters) printf("%d ", plan.polls(iters));
        printf("\n");
        return 0;
    }
    if (argc != 5 || strcmp(argv[1], "plan")) { fprintf(stderr, "usage: see the head of launch_plan_check.cpp\n"); return 2; }
    const LaunchPlan plan = plan_of(argv[2], atoi(argv[3]));
    const int iters = atoi(argv[4]);
    std::vector<int> batches, samples, by_position;
    int it = 0;
    for (int batch = plan.first; it < iters; it += batch, batch = plan.next(batch)) {      // the loop of cg_host.h: a batch is enqueued while the stop word is clear
        batches.push_back(batch);
        const int n = LaunchPlan::counted_slots(it, batch, iters);                         // what the poll after the batch harvests
        for (int q = 0; q < n; ++q) samples.push_back(it + q * LaunchPlan::SAMPLE_STRIDE);
        for (int b = 0; b < batch; ++b)                                                    // the same from the rule of one launch: they must agree
            if (LaunchPlan::sampled(b) && it + b < iters) { by_position.push_back(it + b); if (LaunchPlan::slot(b) >= LaunchPlan::SAMPLE_SLOTS) return 3; }
    }
    if (samples != by_position) { fprintf(stderr, "counted_slots disagrees with sampled / slot\n"); return 3; }
    printf("batches");
    for (int b : batches) printf(" %d", b);
    printf("\npolls %d\nsamples", plan.polls(iters));
    for (int s : samples) printf(" %d", s);
    printf("\n");
    return 0;
}
