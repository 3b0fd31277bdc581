// Host-side choice of the W4 lean compress kernel (ct_quant_pack, ct_quant.hip): a pure function of the launch's size, the input's
// alignment and — in the diagnostics build only — the value of the environment variable CT_W4_COMPRESS.  Plain C++ with no HIP in it,
// so that a stand-alone program can check it (tests/native/w4_variant_check.cpp, built with the host sanitizers by
// tests/test_w4_compress_variant.py).
#pragma once

#include <cstdint>
#include <cstring>

namespace ct {

enum W4CompressVariant {
    kW4CompressPlain = 0,  // w4_quant_pack_lean_kernel: four 16-byte loads per lane, 64 bytes apart
    kW4CompressLds = 1,    // w4_quant_pack_lds_kernel: the wave's 4 KiB by four non-temporal LDS-DMA loads, read back at the lane's own 64 bytes
    kW4CompressBad = -1,   // CT_W4_COMPRESS holds something else: the call fails, it does not guess
};

constexpr int64_t kW4RoundLanes = (int64_t)256 * 8 * 256;  // one residency round of the chip: 256 CUs x 8 workgroups x 256 lanes (kCUs, kBlock)

// `forced` is the variable's value (NULL or "" = unset = "auto"); `lanes` = elements / 32, one lane of either kernel each.
// The LDS form needs one whole wave at least and the 16-byte alignment ct_quant_pack's lean branch already asks for; "lds" takes it
// wherever it can run, "auto" where it was measured to win — HBM-cold, bf16 g128 with int8 zero points, plain / LDS us, medians of 5
// interleaved alternations on one lease (profiles/w4_compress_lds_ab.txt):
//     4096^2 (1 round of lanes)      8.85 /  8.97  the tensor is resident at once: the LDS round trip is latency nothing hides
//     5120^2 (1.6)                  12.74 / 12.58
//     8192^2 (4)                    29.42 / 29.26  and the two-stream step of bench.py, where the decompress co-runs for 45 of its 56 us,
//                                                  5982 -> 6265 GB/s: a once-read stream that does not allocate leaves the caches to the other kernel
//     4096 x 28672 (7)              50.44 / 50.02
// Only 8192^2 cleared the bar set for shipping (more than three min-max spreads, on the step), so the rule starts there.
inline int w4_compress_variant(const char* forced, int64_t lanes, uintptr_t x_addr) {
    const bool lds_ok = lanes >= 64 && (x_addr & 15u) == 0;
    if (forced == nullptr || forced[0] == '\0' || std::strcmp(forced, "auto") == 0)
        return lds_ok && lanes >= 4 * kW4RoundLanes ? kW4CompressLds : kW4CompressPlain;
    if (std::strcmp(forced, "plain") == 0) return kW4CompressPlain;
    if (std::strcmp(forced, "lds") == 0) return lds_ok ? kW4CompressLds : kW4CompressPlain;
    return kW4CompressBad;
}

}  // namespace ct
