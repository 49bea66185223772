// Host-only check of csrc/box_plan.cpp (built from this file and box_plan.cpp alone, with the address and undefined-behaviour sanitizers:
// tests/test_box_plan_host.py).  Reads lines "kernel nx ny nz part_cap" from standard input and prints one line for each: the list of
// box_plan_candidates as "threads q ty cz" groups separated by ';' (an empty list prints an empty line).  A listed plan that
// box_plan_refusal rejects ends the program with exit status 1 and the reason on standard error.
#include <cstdio>

#include "box_plan.hpp"

using namespace sparsh;

int main()
{
    int kernel, nx, ny, nz, part_cap, line = 0;
    while (std::scanf("%d %d %d %d %d", &kernel, &nx, &ny, &nz, &part_cap) == 5) {
        ++line;
        const std::vector<BoxPlan> c = box_plan_candidates(kernel, nx, ny, nz, part_cap);
        for (size_t i = 0; i < c.size(); ++i) {
            const BoxPlan &p = c[i];
            if (const char *why = box_plan_refusal(kernel, nx, ny, nz, p)) {
                std::fprintf(stderr, "line %d: candidate %d %d %d %d refused: %s\n", line, p.threads, p.q, p.ty, p.cz, why);
                return 1;
            }
            std::printf("%s%d %d %d %d", i ? ";" : "", p.threads, p.q, p.ty, p.cz);
        }
        std::printf("\n");
    }
    return 0;
}
