// Stand-alone check of csrc/result_table.h (tests/test_result_table.py compiles it with -fsanitize=address,undefined and reads its output).
//   result_table_check copy <held> <capacity> <mask> [shrink <fewer> | clear]
// A table of 3 int and 2 double columns is sized to <held> rows and filled: int column c holds 100 * c + row, double column c holds c + row / 8 + 0.5.
// "shrink <fewer>": it is then resized to <fewer> rows and those are filled anew with 1000 more; "clear": it is cleared.  Then copy_out at
// <capacity> into buffers of EXACTLY the rows it has to deliver -- one element more written is an AddressSanitizer report --, where bit c of
// <mask> makes int column c NULL, bit 3 + c double column c, and bit 5 rows_out.  Printed: the rows reported, then every column as delivered.
//   result_table_check ints <held> <capacity>          the same for a table of 2 int columns and no double one (the short form of copy_out)
#include "result_table.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

template <int NI, int ND>
static void fill(ResultTable<NI, ND> &t, size_t rows, int shift)
{
    t.resize(rows);
    for (int c = 0; c < NI; ++c)
        for (size_t r = 0; r < rows; ++r) t.i[c][r] = shift + 100 * c + (int)r;
    for (int c = 0; c < ND; ++c)
        for (size_t r = 0; r < rows; ++r) t.d[c][r] = shift + c + (double)r / 8 + 0.5;
}

static void print(const char *name, int c, const int *v, size_t rows)
{
    printf("%s%d", name, c);
    if (!v) printf(" -");
    for (size_t r = 0; v && r < rows; ++r) printf(" %d", v[r]);
    printf("\n");
}
static void print(const char *name, int c, const double *v, size_t rows)
{
    printf("%s%d", name, c);
    if (!v) printf(" -");
    for (size_t r = 0; v && r < rows; ++r) printf(" %.4f", v[r]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "ints")) {
        ResultTable<2> t;
        fill(t, (size_t)atoi(argv[2]), 0);
        const size_t want = clamp_rows(atoi(argv[3]), (long long)t.rows, nullptr);
        int *a = new int[want], *b = new int[want], rows = -7;
        t.copy_out(atoi(argv[3]), &rows, {a, b});
        printf("rows %d\n", rows);
        print("i", 0, a, want); print("i", 1, b, want);
        delete[] a; delete[] b;
        return 0;
    }
    if (argc < 5 || strcmp(argv[1], "copy")) { fprintf(stderr, "usage: see the head of result_table_check.cpp\n"); return 2; }
    const int capacity = atoi(argv[3]), mask = atoi(argv[4]);
    ResultTable<3, 2> t;
    fill(t, (size_t)atoi(argv[2]), 0);
    if (argc == 7 && !strcmp(argv[5], "shrink")) fill(t, (size_t)atoi(argv[6]), 1000);
    else if (argc == 6 && !strcmp(argv[5], "clear")) t.clear();
    else if (argc != 5) { fprintf(stderr, "usage: see the head of result_table_check.cpp\n"); return 2; }
    const size_t want = clamp_rows(capacity, (long long)t.rows, nullptr);
    int *iv[3], rows = -7;
    double *dv[2];
    for (int c = 0; c < 3; ++c) iv[c] = (mask >> c) & 1 ? nullptr : new int[want];
    for (int c = 0; c < 2; ++c) dv[c] = (mask >> (3 + c)) & 1 ? nullptr : new double[want];
    t.copy_out(capacity, (mask >> 5) & 1 ? nullptr : &rows, {iv[0], iv[1], iv[2]}, {dv[0], dv[1]});
    if ((mask >> 5) & 1) printf("rows none\n"); else printf("rows %d\n", rows);
    for (int c = 0; c < 3; ++c) { print("i", c, iv[c], want); delete[] iv[c]; }
    for (int c = 0; c < 2; ++c) { print("d", c, dv[c], want); delete[] dv[c]; }
    return 0;
}
