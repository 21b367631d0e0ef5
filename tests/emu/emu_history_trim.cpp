// emu_history_trim.cpp — rust-lz-fear_amd/csrc/lzf_history_trim.h compiled for the host behind a C interface (tests/test_history_trim_cpu.py).
#include "../../rust-lz-fear_amd/csrc/lzf_history_trim.h"

extern "C" {

uint64_t lzf_emu_trim_shift(uint64_t existing, uint64_t out_cap) { return lzf_trim::shift_of(existing, out_cap); }
void lzf_emu_trim(const lzf_decompress_job* job, lzf_decompress_job* trimmed, uint64_t* shift) { *trimmed = lzf_trim::trim(*job, shift); }
void lzf_emu_restore(lzf_job_result* r, uint64_t shift) { lzf_trim::restore(*r, shift); }

}
