// lz4_decode_head_copies.inc — the copies of the head walk (lz4_decode_head_walk.inc), shared by the two kernels that run it:
// lzf_decode_head_kernel (lz4_decode_head.hip) and lzf_frame_head_kernel (frame_device_head.hip).  Textual include at namespace
// scope, inside namespace lzf and the including source's unnamed namespace, behind that source's kOwn (bytes of a run a lane moves
// by itself) and kStep (bytes the wave moves per step).
static_assert(kOwn == 64u, "lane_copy moves a run of up to four 16-byte pieces");
static_assert(kStep == 16u * kWave, "a step of the wave is 16 bytes a lane");

__device__ __forceinline__ void st8(gu8* p, uint64_t v) { reinterpret_cast<LZF_GLOBAL U8B*>(p)->v = v; }
__device__ __forceinline__ void st4(gu8* p, uint32_t v) { reinterpret_cast<LZF_GLOBAL U4B*>(p)->v = v; }
__device__ __forceinline__ void st2(gu8* p, uint32_t v) { reinterpret_cast<LZF_GLOBAL U2B*>(p)->v = (uint16_t)v; }

// One lane: dst[0, n) = src[0, n), n <= kOwn, the ranges apart.  Reads src[0, n) and writes dst[0, n) and nothing else: a piece at
// the front and one that ends with the run (they may overlap: the same bytes), whole pieces in between from 33 bytes on.
__device__ __forceinline__ void lane_copy(gu8* dst, cgu8* src, uint32_t n) {
    if (n >= 16u) {
        const u32x4 a = ld16(src), z = ld16(src + n - 16u);
        u32x4 m0 = a, m1 = a;
        if (n > 32u) m0 = ld16(src + 16u);
        if (n > 48u) m1 = ld16(src + 32u);
        st16(dst, a);
        if (n > 32u) st16(dst + 16u, m0);
        if (n > 48u) st16(dst + 32u, m1);
        st16(dst + n - 16u, z);
    } else if (n >= 8u) {
        const uint64_t a = ld8(src), z = ld8(src + n - 8u);
        st8(dst, a); st8(dst + n - 8u, z);
    } else if (n >= 4u) {
        const uint32_t a = ld4(src), z = ld4(src + n - 4u);
        st4(dst, a); st4(dst + n - 4u, z);
    } else if (n >= 2u) {
        const uint32_t a = ld2(src), z = ld2(src + n - 2u);
        st2(dst, a); st2(dst + n - 2u, z);
    } else if (n == 1u) {
        dst[0] = src[0];
    }
}

// The whole wave, uniform arguments: dst[0, n) = src[0, n), the ranges apart and the source written (and waited for) before the call.
__device__ __forceinline__ void wave_copy_apart(gu8* dst, cgu8* src, uint64_t n, uint32_t lane) {
    uint64_t base = 0;
    for (; n - base >= kStep; base += kStep) st16(dst + base + lane * 16u, ld16(src + base + lane * 16u));
    const uint32_t rest = (uint32_t)(n - base), whole = rest & ~15u;
    if (lane * 16u < whole) st16(dst + base + lane * 16u, ld16(src + base + lane * 16u));
    if (lane < rest - whole) dst[base + whole + lane] = src[base + whole + lane];
}

// The whole wave, uniform arguments: the first nm bytes of a match at output position mo with offset off (off - mo <= plen,
// lzf_size::check).  Everything in front of mo is written and waited for.  The source starts in the prefix's tail where off > mo
// and goes on at out[0]; where the match overlaps itself (off < nm) it is moved in pieces that end in front of what they write,
// with a wait in between — or, for a period below 16, from the period's bytes in two registers, without further loads.
__device__ __forceinline__ void wave_match(gu8* out, cgu8* pre, uint64_t plen, uint64_t mo, uint32_t off, uint64_t nm, uint32_t lane) {
    uint64_t done = 0;
    if ((uint64_t)off > mo) {
        const uint64_t back = (uint64_t)off - mo, np = nm < back ? nm : back;
        wave_copy_apart(out + mo, pre + (plen - back), np, lane);
        done = np;
        if (done == nm) return;
        wave_store_fence();
    }
    if (off >= 16u) {
        while (done < nm) {
            const uint64_t left = nm - done;
            const uint32_t w = left < off ? (uint32_t)left : off;
            wave_copy_apart(out + mo + done, (cgu8*)out + (mo + done - off), w, lane);
            done += w;
            if (done < nm) wave_store_fence();
        }
        return;
    }
    // the period: out[mo + done - off, mo + done), byte k in bits 8k of (lo, hi); every lane reads the same addresses
    cgu8* const p = (cgu8*)out + (mo + done - off);
    uint64_t lo = 0, hi = 0;
    for (uint32_t k = 0; k < off; ++k) {
        const uint64_t b = p[k];
        if (k < 8u) lo |= b << (8u * k); else hi |= b << (8u * (k - 8u));
    }
    gu8* const d = out + mo + done;
    const uint64_t left = nm - done;
    uint32_t pb = 0;                                   // base % off
    for (uint64_t base = 0; base < left; base += kStep, pb = (pb + kStep) % off) {
        const uint64_t i0 = base + lane * 16u;
        if (i0 >= left) break;
        uint32_t ph = (pb + lane * 16u) % off;
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t b = (uint32_t)((ph < 8u ? lo >> (8u * ph) : hi >> (8u * (ph - 8u))) & 255ull);
            v[j >> 2] |= b << (8u * (j & 3u));
            ph = ph + 1u == off ? 0u : ph + 1u;
        }
        if (left - i0 >= 16u) st16(d + i0, v);
        else {
#pragma unroll
            for (uint32_t j = 0; j < 15u; ++j) if (i0 + j < left) d[i0 + j] = (uint8_t)(v[j >> 2] >> (8u * (j & 3u)));
        }
    }
}
