// ct_plan.h — host side of the table planners (`ct_*_plan`): one loop over a table's items, the magic divisor, the derived fields of a
// `ct_w4_item`.  Host only and free of the HIP runtime: tests/native/plan_check.cpp includes it under the host sanitizers.
#pragma once

#include <stdint.h>

#include "../../include/ct_hip.h"

namespace ct {

void set_error(const char* fmt, ...);

constexpr int64_t kMaxLaunchBlocks = (int64_t)1 << 31;  // a launch takes fewer workgroups than this

// what an entry asks of the loop beyond its name.  Three entries answer an empty table differently from the rest, and keep doing so
// (DESIGN.md 5.25): ct_fp4_batch_plan and ct_mx_scale_batch_plan refuse a NULL table even when n == 0; ct_rtn_nvfp4_batch_plan refuses n <= 0
// with a text of its own.
struct PlanRules {
    bool null_table_is_error = false;   // items == NULL is "bad arguments" whatever n is
    const char* empty_is_error = nullptr;  // n <= 0 is an error with this text (a format taking the entry's name and n)
    bool args_ok = true;                // the entry's own arguments (direction, workspace pointer): false is "bad arguments" too
};

// The plan loop of every table entry: checks (items, n), calls item(items[i], i, first_block) for every item in order — it returns the item's
// workgroup count, or -1 with the error already set — and refuses a table of 2^31 workgroups or more.  Returns the table's count or -1.
template <typename Item, typename F>
int64_t plan_table(const char* name, Item* items, int n, F&& item, const PlanRules& rules = {}) {
    if (rules.empty_is_error && (n <= 0 || items == nullptr)) {
        set_error(rules.empty_is_error, name, n);
        return -1;
    }
    if (n < 0 || (items == nullptr && (n > 0 || rules.null_table_is_error)) || !rules.args_ok) {
        set_error("%s: bad arguments", name);
        return -1;
    }
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t b = item(items[i], i, blocks);
        if (b < 0) return -1;
        blocks = b > INT64_MAX - blocks ? INT64_MAX : blocks + b;  // saturates: the sum is refused below long before, and never overflows
    }
    if (blocks >= kMaxLaunchBlocks) {
        set_error("%s: %lld workgroups exceed one launch; split the batch", name, (long long)blocks);
        return -1;
    }
    return blocks;
}

// n / G as (n * magic) >> shift, exact for 0 <= n < 2^31 (Granlund-Montgomery with N = 31: L = ceil(log2 G), shift = 31 + L,
// magic = ceil(2^shift / G) < 2^32; 2^(31 + L) + G - 1 < 2^63).  False for G < 1 or L > 31, with nothing written.
inline bool magic_div(int64_t G, uint32_t* magic, int32_t* shift) {
    if (G < 1) return false;
    int L = 0;
    while (L <= 31 && ((int64_t)1 << L) < G) ++L;
    if (L > 31) return false;
    *shift = 31 + L;
    *magic = (uint32_t)((((uint64_t)1 << (31 + L)) + (uint64_t)(G - 1)) / (uint64_t)G);
    return true;
}

// the derived fields of a ct_w4_item; g_magic / g_shift are zero unless the item divides by a magic number
inline void fill_w4_item(ct_w4_item& it, int64_t units, int32_t upg, int32_t upg_shift, int64_t first_block, int64_t main_blocks, uint32_t g_magic = 0,
                         int32_t g_shift = 0) {
    it.units = units;
    it.upg = upg;
    it.upg_shift = upg_shift;
    it.first_block = first_block;
    it.main_blocks = main_blocks;
    it.g_magic = g_magic;
    it.g_shift = g_shift;
}

}  // namespace ct
