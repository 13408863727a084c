// result_table.h -- where a filament analysis keeps a table of its result on the host between the find call and the dkmc_copy_* entry points: NI
// int columns and ND double columns of one common row count, and the one copy-out body of those entry points.  Host arithmetic without HIP (the
// standard library only, as launch_plan.h), checked on the CPU under the sanitizers: tests/cpu/result_table_check.cpp, tests/test_result_table.py.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

// rows of a copy-out entry point: min(have, capacity), not below 0, reported in *rows_out
inline size_t clamp_rows(int capacity, long long have, int *rows_out)
{
    long long rows = have < capacity ? have : capacity;
    if (rows < 0) rows = 0;
    if (rows_out) *rows_out = (int)rows;
    return (size_t)rows;
}

template <int NI, int ND = 0>
struct ResultTable {
    size_t rows = 0;
    std::vector<int> i[NI ? NI : 1];
    std::vector<double> d[ND ? ND : 1];

    void clear() { resize(0); }
    // every column at `n` elements; what a row held before is not defined (the find calls write every row they size)
    void resize(size_t n)
    {
        rows = n;
        for (int c = 0; c < NI; ++c) i[c].resize(n);
        for (int c = 0; c < ND; ++c) d[c].resize(n);
    }
    // the first clamp_rows(capacity, rows, rows_out) elements of column c into iout[c] / dout[c]; a NULL column is skipped, and 0 rows touch nothing
    void copy_out(int capacity, int *rows_out, int *const (&iout)[NI ? NI : 1], double *const (&dout)[ND ? ND : 1]) const
    {
        const size_t r = clamp_rows(capacity, (long long)rows, rows_out);
        if (r == 0) return;
        for (int c = 0; c < NI; ++c)
            if (iout[c]) memcpy(iout[c], i[c].data(), r * sizeof(int));
        for (int c = 0; c < ND; ++c)
            if (dout[c]) memcpy(dout[c], d[c].data(), r * sizeof(double));
    }
    void copy_out(int capacity, int *rows_out, int *const (&iout)[NI ? NI : 1]) const
    {
        static_assert(ND == 0, "a table with double columns names them in copy_out");
        double *const none[1] = {nullptr};
        copy_out(capacity, rows_out, iout, none);
    }
};
