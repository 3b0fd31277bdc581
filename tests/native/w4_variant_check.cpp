// Stand-alone caller of ct::w4_compress_variant (csrc/ct_w4_variant.h), built with the host sanitizers by tests/test_w4_compress_variant.py:
//   w4_variant_check <env value or - for unset> <lanes> <address> [...]   prints one decision per triple (plain / lds / bad)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../compressed_tensors_amd/csrc/ct_w4_variant.h"

int main(int argc, char** argv) {
    if ((argc - 1) % 3 != 0) return 2;
    for (int i = 1; i + 2 < argc; i += 3) {
        const std::string env(argv[i]);  // a copy of exactly the value's length: a read past its end is a sanitizer report
        const long long lanes = std::strtoll(argv[i + 1], nullptr, 0);
        const unsigned long long addr = std::strtoull(argv[i + 2], nullptr, 0);
        const int v = ct::w4_compress_variant(env == "-" ? nullptr : env.c_str(), (int64_t)lanes, (uintptr_t)addr);
        std::puts(v == ct::kW4CompressPlain ? "plain" : v == ct::kW4CompressLds ? "lds" : "bad");
    }
    return 0;
}
