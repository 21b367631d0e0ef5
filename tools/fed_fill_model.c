// tools/fed_fill_model.c — how full are the batches of the bitmap-fed decompress kernel, under which window rule?
// A CPU model of the kernel's window loop (lz4_decompress_fed.hip: list the tokens of a window of compressed bytes, form batches of up
// to 64 sequences and at most RING / 3 output bytes from that list) over a file cut into 4 MiB blocks, each compressed with the oracle.
// The window rules are the kernel's own (rust-lz-fear_amd/csrc/lzf_fed_window.h).  Rows:
//   none        no window boundary at all: batches over the whole block's tokens (the batching of tools/round_rules.c)
//   fixed R     R-aligned rounds of R bytes (R = 1024: the kernel before the windows followed the chain)
//   chain C     windows that start at the chain's position (32-aligned), a last batch of <= C sequences left for the next window
// Columns: batches, sequences per batch, batches of fewer than 32 sequences, windows staged.
//   gcc -O2 -o /tmp/fed_fill_model tools/fed_fill_model.c oracle/lzf_oracle.c && /tmp/fed_fill_model /tmp/silesia_mix.bin [blocks]
// ANALYSIS TOOL (links the oracle): not part of the product.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "../oracle/lzf_oracle.h"
#include "../rust-lz-fear_amd/csrc/lzf_fed_window.h"
#define BS (4u << 20)
#define RING 4096u
typedef struct { uint32_t pos, tot; } tok_t;
typedef struct { double batches, seqs, under32, windows; } row_t;
static tok_t* toks; static size_t ntok;
static void parse(const uint8_t* c, size_t len) {
    size_t p = 0; ntok = 0;
    while (p < len) {
        tok_t t; t.pos = (uint32_t)p; uint8_t tok = c[p++]; uint32_t L = tok >> 4, M = 0;
        if (L == 15) { uint8_t b; do { b = c[p++]; L += b; } while (b == 255); }
        p += L;
        if (len - p >= 2) { p += 2; M = tok & 15; if (M == 15) { uint8_t b; do { b = c[p++]; M += b; } while (b == 255); } M += 4; }
        else p = len;
        t.tot = L + M; toks[ntok++] = t;
    }
}
// batches over tokens [i0, i1): returns the index of the first token not put into a batch (a carried tail), i1 when none
static size_t batches_over(size_t i0, size_t i1, uint32_t window_end, uint32_t len, uint32_t carry, row_t* r) {
    const size_t first = i0;
    while (i0 < i1) {
        if (lzf_fedw_carry((uint32_t)(i1 - first), (uint32_t)(i0 - first), window_end, len, carry)) return i0;
        size_t i = i0; uint32_t span = 0;
        while (i < i1 && i - i0 < kFedwLanes) { if (span + toks[i].tot > RING / 3) break; span += toks[i].tot; ++i; }
        if (i == i0) ++i;                                   // a sequence larger than a batch: solo
        r->batches += 1; r->seqs += (double)(i - i0); if (i - i0 < 32) r->under32 += 1;
        i0 = i;
    }
    return i1;
}
static void model(uint32_t len, uint32_t round, int chain, uint32_t carry, row_t* r) {
    if (round == 0) { r->windows += 1; batches_over(0, ntok, len, len, 0, r); return; }
    size_t i = 0;
    while (i < ntok) {
        const uint32_t cstart = chain ? lzf_fedw_start(toks[i].pos, 0) : toks[i].pos / round * round;
        size_t e = i; while (e < ntok && toks[e].pos - cstart < round) ++e;
        r->windows += 1;
        i = batches_over(i, e, cstart + round, len, chain ? carry : 0u, r);
    }
}
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 1;
    fseek(f, 0, SEEK_END); size_t total = ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t* data = malloc(total); if (fread(data, 1, total, f) != total) return 1; fclose(f);
    size_t nblk = (total + BS - 1) / BS; if (argc > 2 && (size_t)atol(argv[2]) < nblk) nblk = atol(argv[2]);
    toks = malloc(sizeof(tok_t) * (BS / 2));
    uint8_t* comp = malloc(BS + 65536);
    static const struct { const char* name; uint32_t round; int chain; uint32_t carry; } rows[] = {
        {"none", 0, 0, 0}, {"fixed 512", 512, 0, 0}, {"fixed 1024", 1024, 0, 0}, {"fixed 2048", 2048, 0, 0}, {"fixed 4096", 4096, 0, 0},
        {"chain 0", kFedwRound, 1, 0}, {"chain 24", kFedwRound, 1, 24}, {"chain 32", kFedwRound, 1, 32}, {"chain 48", kFedwRound, 1, 48}};
    enum { NR = sizeof rows / sizeof rows[0] };
    row_t acc[NR]; memset(acc, 0, sizeof acc);
    for (size_t b = 0; b < nblk; ++b) {
        size_t n = total - b * BS < BS ? total - b * BS : BS, clen = 0;
        lzfo_u32_table t; memset(&t, 0, sizeof t);
        if (lzfo_compress2(data + b * BS, n, 0, LZFO_TABLE_U32, &t, comp, n, &clen) != LZFO_OK) continue;      // (stored blocks are not decompressed)
        parse(comp, clen);
        for (int k = 0; k < NR; ++k) model((uint32_t)clen, rows[k].round, rows[k].chain, rows[k].carry, &acc[k]);
    }
    printf("%-12s %10s %10s %12s %10s\n", "windows", "batches", "seq/batch", "under 32", "staged");
    for (int k = 0; k < NR; ++k)
        printf("%-12s %10.0f %10.1f %11.1f%% %10.0f\n", rows[k].name, acc[k].batches, acc[k].seqs / acc[k].batches, 100.0 * acc[k].under32 / acc[k].batches, acc[k].windows);
    return 0;
}
