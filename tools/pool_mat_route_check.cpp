// Stand-alone check of the host side of wesup_sp_pool_mat_fwd / _bwd (wesup_amd/csrc/pool_mat_route.hpp): the size rule, its
// environment override and the operand checks, over the shapes of the step, of tests/test_pool_mat_sparse_gpu.py and the
// rejected ones.  No GPU and no HIP:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/pool_mat_route_check.cpp -o /tmp/pool_mat_route_check && /tmp/pool_mat_route_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../wesup_amd/csrc/pool_mat_route.hpp"

static int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    unsetenv("WESUP_POOL_MAT_SPARSE_MIN");
    // the default rule: the pinned 3 x 64 x 48 step (Kmax = 64) stays dense at all four of its resolutions, the benchmark's are sparse
    EXPECT(pool_mat_sparse_min() >= 16384);
    EXPECT(!pool_mat_sparse(64, 32 * 24) && !pool_mat_sparse(64, 16 * 12) && !pool_mat_sparse(64, 8 * 6) && !pool_mat_sparse(64, 4 * 3));
    EXPECT(!pool_mat_sparse(6, 768) && !pool_mat_sparse(1, 1) && !pool_mat_sparse(130, 65) && !pool_mat_sparse(0, 100) && !pool_mat_sparse(100, -1));
    EXPECT(pool_mat_sparse(576, 3600) && pool_mat_sparse(576, 900) && pool_mat_sparse(1536, 2500) && pool_mat_sparse(64, 2304));
    EXPECT(pool_mat_sparse(65535, 8192) && pool_mat_sparse(2147483647, 8192));          // the product is taken in 64 bits
    setenv("WESUP_POOL_MAT_SPARSE_MIN", "0", 1);
    EXPECT(!pool_mat_sparse(576, 3600) && !pool_mat_sparse(2147483647, 8192));
    setenv("WESUP_POOL_MAT_SPARSE_MIN", "1", 1);
    EXPECT(pool_mat_sparse(1, 1) && pool_mat_sparse(64, 768) && !pool_mat_sparse(0, 1));
    setenv("WESUP_POOL_MAT_SPARSE_MIN", "2073600", 1);
    EXPECT(pool_mat_sparse(576, 3600) && !pool_mat_sparse(576, 3599));
    setenv("WESUP_POOL_MAT_SPARSE_MIN", "rubbish", 1);
    EXPECT(!pool_mat_sparse(576, 3600));                                                 // atol gives 0: never
    unsetenv("WESUP_POOL_MAT_SPARSE_MIN");

    // operands: real, 16-byte aligned storage for the pointers the checks look at (they are never dereferenced)
    std::vector<float> buf(64);
    float* a = buf.data();
    while (((uintptr_t)a) & 15) ++a;
    const int shapes[][6] = {// B, Kmax, hw, C, ld, off
                             {4, 576, 3600, 768, 2112, 576}, {4, 576, 900, 768, 2112, 1344}, {4, 1536, 2500, 768, 2112, 576},
                             {1, 576, 3600, 768, 2112, 576}, {3, 1, 1, 4, 8, 4}, {3, 65, 63, 260, 2112, 1344},
                             {3, 130, 65, 768, 2112, 1344}, {3, 65, 2049, 4, 2112, 2108}, {2, 1, 65, 1028, 2112, 1084},
                             {1, 64, 4100, 4, 4, 0}, {65535, 1, 8192, 4, 4, 0}};
    for (const auto& sh : shapes)
        EXPECT(pool_mat_operands_ok(a, a, a, a, sh[4], sh[5], sh[0], sh[1], sh[2], sh[3]));
    EXPECT(!pool_mat_operands_ok(nullptr, a, a, a, 2112, 576, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, nullptr, a, a, 2112, 576, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, nullptr, a, 2112, 576, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, nullptr, 2112, 576, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 4, 576, 8193, 768));            // more than 8192 cells
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 4, 576, 8196, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 1348, 4, 576, 3600, 768));           // 1348 + 768 > 2112
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 2147483644, 4, 576, 3600, 768));     // off + C does not wrap
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 764, 0, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, -4, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 578, 4, 576, 3600, 768));            // an offset, a width, a stride off the quad grid
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 4, 576, 3600, 770));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2110, 576, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a + 1, a, 2112, 576, 4, 576, 3600, 768));        // 16-byte loads and stores
    EXPECT(!pool_mat_operands_ok(a, a, a, a + 2, 2112, 576, 4, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 0, 576, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 65536, 576, 3600, 768));        // grid.y
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 4, 0, 3600, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 4, 576, 0, 768));
    EXPECT(!pool_mat_operands_ok(a, a, a, a, 2112, 576, 4, 576, 3600, 0));
    std::printf(failures ? "%d check(s) failed\n" : "pool_mat_route: all checks passed\n", failures);
    return failures ? 1 : 0;
}
