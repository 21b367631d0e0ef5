// capi_analysis.inc — -DLZF_ANALYSIS only (liblzfear_hip_analysis.so): every kernel generation behind the same entry points and
// every tuning value of lzf_dispatch.h's Knobs, selected with environment variables, for A/B timing and counter studies (tools/,
// profiles/).  Included by capi.hip inside its anonymous namespace; nothing here is in the product library.  The environment is
// read ONCE per process, by analysis_knobs() (tests start a child per setting).
enum { kVariantAuto = -1, kVariantWave = 0, kVariantFirstBatched = 1, kVariantFirstPaired = 200 };
static int variant_by_name(const char* e) {
    if (!strcmp(e, "auto")) return kVariantAuto;
    if (!strcmp(e, "wave")) return kVariantWave;
    int id = kVariantFirstBatched;
#define LZF_NAME(NAME, R, S_, T, ST) if (!strcmp(e, #NAME)) return id; ++id;
    LZF_DECOMPRESS_VARIANTS(LZF_NAME)
#undef LZF_NAME
    id = kVariantFirstPaired;
#define LZF_NAMEP(NAME, RG, S_, T) if (!strcmp(e, #NAME)) return id; ++id;
    LZF_PAIRED_VARIANTS(LZF_NAMEP)
#undef LZF_NAMEP
    return kVariantAuto;                       // unknown names select the default
}

// One row per variable: a uint32_t field and the parser of its value (false: the value is refused, the default stays), or a
// function that sets what the variable means.  Rows are applied top to bottom.
struct KnobRow {
    const char* name;
    uint32_t d::Knobs::* field;
    bool (*parse)(const char* e, uint32_t* v);
    void (*set)(const char* e, d::Knobs& k);
};
static bool knob_any(const char* e, uint32_t* v) { *v = (uint32_t)atol(e); return true; }
template <long LO, long HI> static bool knob_in(const char* e, uint32_t* v) { const long x = atol(e); if (x < LO || x > HI) return false; *v = (uint32_t)x; return true; }
static bool knob_order(const char* e, uint32_t* v) { *v = !strcmp(e, "natural") ? d::kOrderNatural : !strcmp(e, "always") ? d::kOrderAlways : d::kOrderByRule; return true; }
static bool knob_ring(const char* e, uint32_t* v) { const long x = atol(e); if (x != 32768 && x != 65536 && x != 131072) return false; *v = (uint32_t)x; return true; }
static bool knob_seg_force(const char* e, uint32_t* v) { *v = !strcmp(e, "stager") ? 1u : !strcmp(e, "resolver") ? 2u : !strcmp(e, "noscratch") ? 3u : !strcmp(e, "swait") ? 8u : 0u; return true; }
static bool knob_compress_kernel(const char* e, uint32_t* v) { *v = !strcmp(e, "general") ? d::kCompressGeneral : !strcmp(e, "compact") ? d::kCompressCompact : d::kCompressByRule; return true; }
static const KnobRow kKnobRows[] = {
    {"LZF_FAKE_CU", &d::Knobs::fake_cu, knob_in<1, 4096>, nullptr},              // dispatch as if the device had n compute units (test of the derived thresholds on one device)
    // auto | wave | a name of the LZF_*_VARIANTS lists of kernels.h: that kernel whatever the batch;  seg / noseg: the pipeline for every call / for none;
    // fed: the bitmap-fed path for every call (and no pipeline) / nofed: for none
    {"LZF_DECOMPRESS_KERNEL", nullptr, nullptr, [](const char* e, d::Knobs& k) {
        if (*e) k.variant = variant_by_name(e);
        if (!strcmp(e, "seg")) { k.seg = d::kForced; k.seg_min_in = 0u; }
        if (!strcmp(e, "noseg") || !strcmp(e, "fed")) k.seg = d::kOff;
        if (!strcmp(e, "fed")) k.fed = d::kForced;
        if (!strcmp(e, "nofed")) k.fed = d::kOff; }},
    {"LZF_DECOMPRESS_ORDER", &d::Knobs::decompress_order, knob_order, nullptr},  // natural | always (default: longest first beyond one residency)
    {"LZF_COMPRESS_ORDER", &d::Knobs::compress_order, knob_order, nullptr},
    {"LZF_ORDER_LEN_SHIFT", &d::Knobs::order_len_shift, knob_any, nullptr},      // the decompress estimate + input length >> k (A/B of the cost proxy)
    {"LZF_COMPRESS_KERNEL", &d::Knobs::compress_kernel, knob_compress_kernel, nullptr},      // general (everything on lzf_compress_wave_kernel) | compact (no latency class)
    {"LZF_COMPRESS_TEAM_MAX", nullptr, nullptr, [](const char* e, d::Knobs& k) { const long v = atol(e); if (v >= 0) k.team_max = v; }},      // jobs per call the team kernel takes
    {"LZF_COMPACT_PAD_LDS", &d::Knobs::compact_pad_lds, knob_any, nullptr},      // bytes of unused LDS per wavefront: fewer resident waves per CU (the residency experiment)
    {"LZF_PROBE", nullptr, nullptr, [](const char* e, d::Knobs& k) {             // "piece,parts": the cost probe's sample (A/B of the launch order's estimate)
        unsigned a = 0, b = 0; if (sscanf(e, "%u,%u", &a, &b) == 2 && a >= 4096u && b >= 1u && b <= 16u) { k.probe_piece = a; k.probe_parts = b; } }},
    {"LZF_SEG_FORCE", &d::Knobs::seg_force, knob_seg_force, nullptr},            // noscratch | stager | resolver | swait: the pipeline's fall-backs, forced (tests/test_gpu_parity.py)
    {"LZF_SEG_RING", &d::Knobs::seg_ring, knob_ring, nullptr},                   // a ring size whatever the batch (one block per CU with the small rings: the stager's share)
    {"LZF_SEG_GRID", nullptr, nullptr, [](const char* e, d::Knobs& k) {          // "parse,tiles": workgroups per launch of the chunk / tile kernels (A/B of the grid sizes)
        unsigned a = 0, b = 0; if (sscanf(e, "%u,%u", &a, &b) == 2 && a && b) { k.seg_grid_parse = a; k.seg_grid_tile = b; } }},
    {"LZF_SEG_REC_PAD", &d::Knobs::seg_rec_pad, knob_any, nullptr},              // bytes of unused LDS per workgroup of a grouped call's records stage (fewer of them resident under the resolve stages: A/B)
    {"LZF_SEG_GROUPS", nullptr, nullptr, [](const char* e, d::Knobs& k) {        // "a,b,c,...": per cent of the jobs per group (A/B of the grouping; "100" = one group)
        uint32_t v[d::kSegMaxGroups] = {}, got = 0, sum = 0; const char* q = e;
        while (got < d::kSegMaxGroups && *q) { char* end = nullptr; const unsigned long x = strtoul(q, &end, 10); if (end == q) break; v[got++] = (uint32_t)x; sum += (uint32_t)x; q = *end == ',' ? end + 1 : end; if (*end != ',') break; }
        if (got >= 1 && sum == 100u && v[0]) { for (uint32_t i = 0; i < d::kSegMaxGroups; ++i) k.seg_group_pct[i] = v[i]; k.seg_group_n = got; } }},
    {"LZF_SEG_MIN_IN", nullptr, nullptr, [](const char* e, d::Knobs& k) { if (k.seg == d::kForced) k.seg_min_in = (uint32_t)atol(e); }},      // the forced pipeline's smallest input (LZF_DECOMPRESS_KERNEL=seg, above: 0)
    // the smallest input the bitmap-fed kernel takes; set at all, it opens the path to calls whose inputs the caller bounds (the variant parity test opens it to every input)
    {"LZF_FED_MIN_IN", nullptr, nullptr, [](const char* e, d::Knobs& k) { const long v = atol(e); if (v >= 0) k.fed_min_in = (uint32_t)v; k.fed_open = true; }},
    {"LZF_FED_PIECES", &d::Knobs::fed_pieces, knob_in<1, 4096>, nullptr},        // pieces per job (A/B)
    {"LZF_FED_SLOTS", &d::Knobs::fed_slots, knob_in<1, 0x7FFFFFFFL>, nullptr},   // slots per CU
    {"LZF_FED_PAD_LDS", &d::Knobs::fed_pad_lds, knob_any, nullptr},              // bytes of unused LDS per wavefront (residency experiment)
    {"LZF_FED_CARRY", &d::Knobs::fed_carry, knob_in<0, 63>, nullptr},            // the longest last batch of a window that is left for the next window (0: never; A/B)
    // the size call's latency class: force = every call that fits its scratch / off = none; its smallest input; LZF_SIZE_FORCE=1 its scratch
    // refused, 2 no one-wave kernel behind it (tests/test_gpu_size_latency.py: what the class finished itself)
    {"LZF_SIZE_SEG", nullptr, nullptr, [](const char* e, d::Knobs& k) { k.size_seg = !strcmp(e, "force") ? d::kForced : !strcmp(e, "off") ? d::kOff : d::kByRule; }},
    {"LZF_VERIFY_SEG", nullptr, nullptr, [](const char* e, d::Knobs& k) { k.verify_seg = !strcmp(e, "force") ? d::kForced : !strcmp(e, "off") ? d::kOff : d::kByRule; }},
    {"LZF_SIZE_SEG_MIN_IN", &d::Knobs::size_seg_min_in, knob_any, nullptr},
    {"LZF_SIZE_FORCE", &d::Knobs::size_force, knob_in<0, 2>, nullptr},
    {"LZF_FED_VERBOSE", nullptr, nullptr, [](const char*, d::Knobs& k) { k.fed_verbose = true; }},
};
static d::Knobs analysis_knobs() {
    d::Knobs k;
    for (const KnobRow& r : kKnobRows) {
        const char* e = getenv(r.name);
        if (!e) continue;
        uint32_t v = 0;
        if (r.set) r.set(e, k);
        else if (r.parse(e, &v)) k.*r.field = v;
    }
    return k;
}

// every launch below is checked: one LAUNCH per variant
static int analysis_launch_decompress(int variant, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, const uint32_t* cperm, hipStream_t st) {
    if (variant == kVariantWave) {
        LAUNCH(lzf::lzf_decompress_wave_kernel, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, cperm);
    } else if (variant < kVariantFirstPaired) {
        int id = kVariantFirstBatched;
#define LZF_LAUNCH(NAME, R, S_, T, ST) \
        if (variant == id++) LAUNCH((lzf::lzf_decompress_batched_kernel<R, S_, T, ST>), dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, cperm);
        LZF_DECOMPRESS_VARIANTS(LZF_LAUNCH)
#undef LZF_LAUNCH
    } else {
        int id = kVariantFirstPaired;
#define LZF_LAUNCHP(NAME, RG, S_, T) \
        if (variant == id++) LAUNCH((lzf::lzf_decompress_paired_kernel<RG, S_, T>), dim3(n_jobs), dim3(128), 0, st, d_jobs, d_results, n_jobs, cperm, (const lzf::seg_job*)nullptr);
        LZF_PAIRED_VARIANTS(LZF_LAUNCHP)
#undef LZF_LAUNCHP
    }
    return LZF_OK;
}
