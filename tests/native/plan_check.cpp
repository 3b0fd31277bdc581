// Stand-alone check of csrc/ct_plan.h under the host sanitizers (built and run by tests/test_plan_tables.py; no HIP runtime, nothing loaded into
// python): magic_div against plain division, and the plan loop on a dummy item type up to its 2^31 refusal.  Prints "ok" or the first mismatch.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../compressed_tensors_amd/csrc/ct_plan.h"

static char g_error[512];
void ct::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int check_divisor(int64_t G) {
    uint32_t magic = 0xdeadbeefu;
    int32_t shift = -1;
    CHECK(ct::magic_div(G, &magic, &shift), "magic_div refused G = %lld", (long long)G);
    CHECK(shift >= 31 && shift <= 62, "G = %lld: shift %d", (long long)G, shift);
    const uint64_t probes[] = {0, (uint64_t)(G - 1), (uint64_t)G, ((uint64_t)1 << 31) - 1};
    for (uint64_t n : probes) {
        if (n >= ((uint64_t)1 << 31)) continue;  // exact for n < 2^31 only
        CHECK(((n * magic) >> shift) == n / (uint64_t)G, "G = %lld, n = %llu: %llu != %llu", (long long)G, (unsigned long long)n,
              (unsigned long long)((n * magic) >> shift), (unsigned long long)(n / (uint64_t)G));
    }
    return 0;
}

struct Dummy {
    int64_t blocks, first_block;
};

static int64_t dummy_item(Dummy& it, int i, int64_t first_block) {
    if (it.blocks < 0) {
        ct::set_error("dummy: item %d", i);
        return -1;
    }
    it.first_block = first_block;
    return it.blocks;
}

int main() {
    for (int64_t G = 1; G <= (1 << 16); ++G)
        if (check_divisor(G)) return 1;
    for (int l = 0; l <= 31; ++l)
        for (int64_t d = -1; d <= 1; ++d)
            if (((int64_t)1 << l) + d >= 1 && ((int64_t)1 << l) + d <= ((int64_t)1 << 31) && check_divisor(((int64_t)1 << l) + d)) return 1;
    uint32_t magic = 7;
    int32_t shift = 7;
    const int64_t refused[] = {0, -1, INT64_MIN, ((int64_t)1 << 31) + 1, (int64_t)1 << 32, (int64_t)1 << 62, INT64_MAX};
    for (int64_t G : refused)
        CHECK(!ct::magic_div(G, &magic, &shift) && magic == 7 && shift == 7, "magic_div took G = %lld or wrote its outputs", (long long)G);

    const int64_t half = (int64_t)1 << 30;
    Dummy t[4] = {{half, -1}, {half - 1, -1}, {0, -1}, {1, -1}};
    CHECK(ct::plan_table("dummy_plan", t, 3, dummy_item) == 2 * half - 1, "2^31 - 1 workgroups were refused: %s", g_error);
    CHECK(t[0].first_block == 0 && t[1].first_block == half && t[2].first_block == 2 * half - 1, "first_block");
    CHECK(ct::plan_table("dummy_plan", t, 4, dummy_item) == -1 && !std::strcmp(g_error, "dummy_plan: 2147483648 workgroups exceed one launch; split the batch"),
          "2^31 workgroups: %s", g_error);
    Dummy big[6] = {{INT64_MAX / 4, -1}, {INT64_MAX / 4, -1}, {INT64_MAX / 4, -1}, {INT64_MAX / 4, -1}, {INT64_MAX / 4, -1}, {INT64_MAX, -1}};  // the sum saturates
    CHECK(ct::plan_table("dummy_plan", big, 6, dummy_item) == -1 && std::strstr(g_error, "exceed one launch") && big[5].first_block == INT64_MAX, "a huge table: %s", g_error);
    t[1].blocks = -5;
    CHECK(ct::plan_table("dummy_plan", t, 4, dummy_item) == -1 && !std::strcmp(g_error, "dummy: item 1"), "an item's refusal: %s", g_error);
    t[1].blocks = 1;
    CHECK(ct::plan_table("dummy_plan", t, 0, dummy_item) == 0 && ct::plan_table("dummy_plan", (Dummy*)nullptr, 0, dummy_item) == 0, "an empty table");
    CHECK(ct::plan_table("dummy_plan", t, -1, dummy_item) == -1 && !std::strcmp(g_error, "dummy_plan: bad arguments"), "n = -1: %s", g_error);
    CHECK(ct::plan_table("dummy_plan", (Dummy*)nullptr, 1, dummy_item) == -1 && !std::strcmp(g_error, "dummy_plan: bad arguments"), "(NULL, 1): %s", g_error);
    ct::PlanRules strict;
    strict.null_table_is_error = true;
    CHECK(ct::plan_table("dummy_plan", (Dummy*)nullptr, 0, dummy_item, strict) == -1 && ct::plan_table("dummy_plan", t, 0, dummy_item, strict) == 0, "null_table_is_error");
    ct::PlanRules nonempty;
    nonempty.empty_is_error = "%s: bad arguments (a table of %d items)";
    CHECK(ct::plan_table("dummy_plan", t, 0, dummy_item, nonempty) == -1 && !std::strcmp(g_error, "dummy_plan: bad arguments (a table of 0 items)"), "empty_is_error: %s", g_error);
    CHECK(ct::plan_table("dummy_plan", t, 1, dummy_item, nonempty) == half, "empty_is_error on a table");
    ct::PlanRules bad;
    bad.args_ok = false;
    CHECK(ct::plan_table("dummy_plan", t, 1, dummy_item, bad) == -1 && !std::strcmp(g_error, "dummy_plan: bad arguments"), "args_ok: %s", g_error);

    ct_w4_item it;
    std::memset(&it, 0x5a, sizeof it);
    ct::fill_w4_item(it, 11, 2, 1, 3, 4);
    CHECK(it.units == 11 && it.upg == 2 && it.upg_shift == 1 && it.first_block == 3 && it.main_blocks == 4 && it.g_magic == 0 && it.g_shift == 0, "fill_w4_item");
    ct::fill_w4_item(it, 11, 2, 1, 3, 4, 9u, 33);
    CHECK(it.g_magic == 9u && it.g_shift == 33, "fill_w4_item with a magic divisor");
    std::puts("ok");
    return 0;
}
