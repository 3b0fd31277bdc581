// ct_hadamard_block.inc — the butterfly of one workgroup-sized block, n = 64 * WAVES * U * 8, on the values a thread holds: the body of
// had_block_kernel (ct_hadamard.hip), hadk_block_kernel (ct_hadamard_k.hip), hadp_block_kernel (ct_hadamard_perm.hip) and
// rot_block_kernel (ct_rotated.hip), included between their loads and their stores.  Text, not a function: as a __forceinline__ device
// function template the same lines schedule and allocate differently in most of those kernels (DESIGN.md 5.28), and several sit at the
// register limit.
//
// Expects in scope
//   A              the accumulator type, float or double
//   U, WAVES, T    units per thread, waves per workgroup, T = 64 * WAVES (constants)
//   CH, CPU        elements of a 16-byte chunk of A and chunks per unit: 16 / sizeof(A) and 8 / CH (constants)
//   chunk_t        A __attribute__((ext_vector_type(CH)))
//   A v[U][8]      unit u of thread t holds elements ((u * T + t) * 8 ..+8) of the block; transformed in place
//   chunk_t* lds   N / CH chunks of LDS for WAVES > 1 (not touched for one wave): chunk c of unit u of thread t at ((u * CPU + c) * T + t),
//                  consecutive lanes 16 bytes apart for the writes and for the reads
//   tid, lane, wave   threadIdx.x, tid & 63, and tid >> 6 as a wave-uniform value (readfirstlane)
// Stages: the element bits inside a unit and the lane bits of every unit (no LDS), the additions between the U units, then ONE exchange
// between the waves: every thread reads the other waves' value at its own position and adds it with the sign (-1)^popcount(w & wave).
// Barriers (WAVES > 1 only): one between the writes and the reads of the exchange, and it ENDS with one after the reads — whatever the caller
// does to lds next (the next block's exchange, an image laid over it) is already ordered behind them.  A caller that has lds hold something
// else before the body puts its own barrier in front.
// U >= 8: one unit's exchanges at a time — 64 values per thread leave no room for more, so a scheduling barrier stands after each unit's
// lane exchanges and after each chunk of the wave exchange (and the callers put one after each unit's store).
#pragma unroll
for (int u = 0; u < U; ++u) {
    unit_stages(v[u], 8);
    lane_stages(v[u], 64, lane);
    if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
}
#pragma unroll
for (int h = 1; h < U; h <<= 1) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!(u & h)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const A a = v[u][k], c = v[u | h][k];
                v[u][k] = a + c;
                v[u | h][k] = a - c;
            }
        }
    }
}
if constexpr (WAVES > 1) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < CPU; ++c) {
            chunk_t w;
#pragma unroll
            for (int e = 0; e < CH; ++e) w[e] = v[u][c * CH + e];
            lds[(u * CPU + c) * T + tid] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < CPU; ++c) {
            chunk_t r = lds[(u * CPU + c) * T + lane];  // wave 0: sign + for every reader
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                const chunk_t o = lds[(u * CPU + c) * T + w * 64 + lane];
                const A sign = (__builtin_popcount(w & wave) & 1) ? (A)-1 : (A)1;  // wave-uniform
#pragma unroll
                for (int e = 0; e < CH; ++e) r[e] = fma_t(o[e], sign, r[e]);
            }
#pragma unroll
            for (int e = 0; e < CH; ++e) v[u][c * CH + e] = r[e];
            if constexpr (U >= 8) __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
}
