// emu_ring_split.cpp — TEST INFRASTRUCTURE: the (head, vector, tail) split by which the decompress kernels move a range of their
// output ring to or from `out`, as the kernels themselves compile it (rust-lz-fear_amd/csrc/lzf_out_ring.h: lzf_ring_split, used
// by OutRing::fill and OutRing::flush), on the CPU — so that the Python model of the alignment sweep
// (tests/alignment_cases.py::ring_flush_split) can be held against the rule itself.
//   g++ -O2 -std=c++17 -fPIC -shared -o libemu_ring_split.so tests/emu/emu_ring_split.cpp
#include <cstddef>
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_out_ring.h"

// the rule is a constant expression: a whole head in front of one vector store and a tail, and a head clamped to the range
static_assert(lzf_ring_split(0u, 40u, 9u).head == 7u && lzf_ring_split(0u, 40u, 9u).vec == 2u && lzf_ring_split(0u, 40u, 9u).tail == 1u, "");
static_assert(lzf_ring_split(3u, 5u, 0u).head == 2u && lzf_ring_split(3u, 5u, 0u).vec == 0u && lzf_ring_split(3u, 5u, 0u).tail == 0u, "");

// parts[((rb * n_a + a) * n_len + n) * 3 + k] = head, vec, tail of out[a, a + n) at bias rb, for rb < 16, a < n_a, n < n_len
extern "C" void lzf_emu_ring_split_sweep(uint32_t n_a, uint32_t n_len, uint32_t* parts) {
    for (uint32_t rb = 0; rb < 16u; ++rb)
        for (uint32_t a = 0; a < n_a; ++a)
            for (uint32_t n = 0; n < n_len; ++n) {
                const lzf_ring_parts s = lzf_ring_split(a, a + n, rb);
                uint32_t* p = parts + (((size_t)rb * n_a + a) * n_len + n) * 3u;
                p[0] = s.head; p[1] = s.vec; p[2] = s.tail;
            }
}
