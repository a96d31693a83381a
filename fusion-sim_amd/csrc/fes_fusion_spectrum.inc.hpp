// fes_fusion_spectrum.inc.hpp: the fusion product spectra of a CART3D handle (fpic_fusion_spectrum,
// fpic_fusion_spectrum_register, fpic_fusion_spectrum_read, fpic_fusion_spectrum_clear) — part of fes_api.hip's translation
// unit (included there after fes_fusion.inc.hpp, inside namespace fes).  The rule and the checks of a request are
// fes_fusion_spectrum_core.hpp on top of fes_fusion_core.hpp, the pass fes_fusion_spectrum_kernels.hpp.
//
// One application: per species of the request fpic_pair's cell index (pair_index<T>, into the Diag's index buffers,
// unchanged), then the spectrum pass — all enqueued on the handle's stream, nothing read back.  The count words, the tables
// and the histogram words belong to the handle's Diag and are released with it: slot k < FPIC_FUSION_SPECTRUM_MAX_OPS serves
// the k-th registered operator, slot FPIC_FUSION_SPECTRUM_MAX_OPS the call.  A table is uploaded at the call or at the
// registration (which waits for the copy); the hook never allocates, never waits and never reads back.
// A handle with a Domain is refused as fpic_fusion refuses it.

constexpr int kFspecNow = FPIC_FUSION_SPECTRUM_MAX_OPS;      // the slot of fpic_fusion_spectrum
constexpr size_t kFspecSlotWords = static_cast<size_t>(kFspecEntriesMax) * 2;

static int fspec_slots(fpic_handle* h)
{
    Diag& g = h->es->diag;
    void* p = nullptr;
    if (!g.fspec) {
        const size_t bytes = static_cast<size_t>(FPIC_FUSION_SPECTRUM_MAX_OPS + 1) * kFusionWords * sizeof(unsigned long long);
        if (int rc = dev_alloc(h, &p, bytes, &h->bytes_grid)) return rc;
        g.fspec = static_cast<unsigned long long*>(p);
        HIP_TRY(h, hipMemsetAsync(g.fspec, 0, bytes, h->stream));
    }
    if (!g.fspec_table) {
        if (int rc = dev_alloc(h, &p, static_cast<size_t>(FPIC_FUSION_SPECTRUM_MAX_OPS + 1) * FPIC_FUSION_TABLE_MAX * sizeof(double), &h->bytes_grid)) return rc;
        g.fspec_table = static_cast<double*>(p);
    }
    if (!g.fspec_words) {
        const size_t bytes = static_cast<size_t>(FPIC_FUSION_SPECTRUM_MAX_OPS + 1) * kFspecSlotWords * sizeof(unsigned long long);
        if (int rc = dev_alloc(h, &p, bytes, &h->bytes_grid)) return rc;
        g.fspec_words = static_cast<unsigned long long*>(p);
        HIP_TRY(h, hipMemsetAsync(g.fspec_words, 0, bytes, h->stream));
    }
    return FPIC_OK;
}

// the slot starts from zero with the request's table, in stream order; returns after the table has been copied
static int fspec_begin(fpic_handle* h, int slot, const fpic_fusion_spec& tally)
{
    Diag& g = h->es->diag;
    if (int rc = fspec_slots(h)) return rc;
    HIP_TRY(h, hipMemsetAsync(g.fspec + slot * kFusionWords, 0, kFusionWords * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(g.fspec_words + slot * kFspecSlotWords, 0, kFspecSlotWords * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemcpyAsync(g.fspec_table + static_cast<size_t>(slot) * FPIC_FUSION_TABLE_MAX, tally.sigma, static_cast<size_t>(tally.n) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

template <typename T, bool LIKE>
static void fspec_launch(fpic_handle* h, const FspecArgs<T>& a, unsigned grid)
{
    // (the LDS stays below the 64 KiB a launch may ask for without an attribute: the kernels' header asserts it)
    const size_t lds = fspec_lds_bytes(a.s.bins);
    if (a.s.axis == FPIC_FSPEC_CM) fusion_spectrum_kernel<T, LIKE, FPIC_FSPEC_CM><<<grid, kPairThreads, lds, h->stream>>>(a);
    else fusion_spectrum_kernel<T, LIKE, FPIC_FSPEC_PRODUCT><<<grid, kPairThreads, lds, h->stream>>>(a);
}

// one application of the rules (r, s) into `slot`: enqueued, nothing waited for
template <typename T>
static int fspec_enqueue(fpic_handle* h, const fpic_fusion_spec& spec, const fesfusion::Rule& r, const fesfspec::Rule& s, int slot, bool may_grow)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = fusion_buffers(h, spec, may_grow)) return rc;
    const Species& sa = st->sp[spec.species_a];
    const Species& sb = st->sp[spec.species_b];
    const bool like = spec.species_a == spec.species_b;
    if (!sa.n || !sb.n || !(r.s_max > 0)) return FPIC_OK;   // (nothing can react: nothing is launched)
    if (int rc = pair_index<T>(h, sa, 0)) return rc;
    if (!like)
        if (int rc = pair_index<T>(h, sb, 1)) return rc;
    FspecArgs<T> a{};
    a.slab_a = static_cast<const T*>(sa.slab[sa.cur]);
    a.slab_b = static_cast<const T*>(sb.slab[sb.cur]);
    a.id_a = sa.ids_identity ? nullptr : sa.id[sa.cur];
    a.id_b = sb.ids_identity ? nullptr : sb.id[sb.cur];
    a.n_pad_a = sa.n_pad;
    a.n_pad_b = sb.n_pad;
    a.seg_a = g.pair_seg[0] + kPairSegLead - 1;
    a.seg_b = g.pair_seg[like ? 0 : 1] + kPairSegLead - 1;
    a.index_a = g.pair_index[0];
    a.index_b = g.pair_index[like ? 0 : 1];
    a.ncells = static_cast<uint32_t>(pair_cells(st));
    a.rank_max = (pair_forms() & 2) ? static_cast<uint32_t>(kPairRankMax) : ~0u;
    a.counts = g.fspec + slot * kFusionWords;
    a.words = g.fspec_words + slot * kFspecSlotWords;
    a.table = g.fspec_table + static_cast<size_t>(slot) * FPIC_FUSION_TABLE_MAX;
    a.r = r;
    a.s = s;
    const size_t nchunks = (pair_cells(st) + kPairChunk - 1) / kPairChunk;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(kPairCollideBlocks, nchunks));
    if (like) fspec_launch<T, true>(h, a, grid);
    else fspec_launch<T, false>(h, a, grid);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int fspec_apply(fpic_handle* h, const fpic_fusion_spec& spec, const fesfusion::Rule& r, const fesfspec::Rule& s, int slot, bool may_grow)
{
    return h->prec == FPIC_F32 ? fspec_enqueue<float>(h, spec, r, s, slot, may_grow) : fspec_enqueue<double>(h, spec, r, s, slot, may_grow);
}

static int fspec_check(fpic_handle* h, const fpic_fusion_spectrum_spec* spec)
{
    State* st = h->es;
    if (const char* why = fesfspec::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (const char* why = fesfusion::check_bound(spec->tally, st->W, fusion_dv(st))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    return FPIC_OK;
}

static fesfspec::Rule fspec_rule(const State* st, const fpic_fusion_spectrum_spec& spec)
{
    return fesfspec::rule_of(spec, st->sp[spec.tally.species_a].mass, st->sp[spec.tally.species_b].mass);
}

// the slot's counts and words -> out, words ((bins + 2) x 2, every entry joined); waits for the copies
static int fspec_fetch(fpic_handle* h, int slot, int bins, uint64_t applications, int e, fpic_fusion_result* out, uint64_t* words, bool reset)
{
    Diag& g = h->es->diag;
    uint64_t got[kFusionWords] = {};
    const size_t nwords = static_cast<size_t>(bins + 2) * 2;
    HIP_TRY(h, hipMemcpyAsync(got, g.fspec + slot * kFusionWords, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    if (words) HIP_TRY(h, hipMemcpyAsync(words, g.fspec_words + slot * kFspecSlotWords, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (reset) {   // (behind the copies, in stream order)
        HIP_TRY(h, hipMemsetAsync(g.fspec + slot * kFusionWords, 0, kFusionWords * sizeof(unsigned long long), h->stream));
        HIP_TRY(h, hipMemsetAsync(g.fspec_words + slot * kFspecSlotWords, 0, kFspecSlotWords * sizeof(unsigned long long), h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (out) fusion_result(out, applications, got, e);
    if (words)
        for (size_t k = 0; k < nwords; k += 2) fesfusion::join(words[k], words[k + 1], words[k], words[k + 1]);
    return FPIC_OK;
}

int fusion_spectrum(fpic_handle* h, const fpic_fusion_spectrum_spec* spec, fpic_fusion_result* out, uint64_t* words)
{
    State* st = h->es;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum")) return rc;
    if (int rc = fspec_check(h, spec)) return rc;
    if (out) *out = fpic_fusion_result{};
    if (int rc = fspec_begin(h, kFspecNow, spec->tally)) return rc;
    const fesfusion::Rule r = fesfusion::rule_of(spec->tally, spec->tally.epoch, st->W, fusion_dv(st));
    if (int rc = fspec_apply(h, spec->tally, r, fspec_rule(st, *spec), kFspecNow, true)) return rc;
    return fspec_fetch(h, kFspecNow, spec->bins, 1, r.e, out, words, false);
}

int fusion_spectrum_register(fpic_handle* h, const fpic_fusion_spectrum_spec* spec, int every, int* index)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum_register")) return rc;
    if (int rc = fspec_check(h, spec)) return rc;
    if (const char* why = fesfspec::check_register(every, static_cast<int>(g.fspec_ops.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = fusion_buffers(h, spec->tally, true)) return rc;   // (sized now: the hook finds them in place and never grows them)
    const int at = static_cast<int>(g.fspec_ops.size());
    if (int rc = fspec_begin(h, at, spec->tally)) return rc;
    FspecOp op{ *spec, every, 0, fesfusion::rule_of(spec->tally, spec->tally.epoch, st->W, fusion_dv(st)), fspec_rule(st, *spec) };
    op.spec.tally.sigma = nullptr;  // (the table is on the device; the caller's need not outlive this call)
    g.fspec_ops.push_back(op);
    if (index) *index = at;
    return FPIC_OK;
}

int fusion_spectrum_read(fpic_handle* h, int index, fpic_fusion_result* out, uint64_t* words, int reset)
{
    Diag& g = h->es->diag;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum_read")) return rc;
    if (const char* why = fesfusion::check_index(index, static_cast<int>(g.fspec_ops.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (!out && !words && !reset) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    FspecOp& op = g.fspec_ops[index];
    const uint64_t applications = op.applications;
    if (reset) op.applications = 0;
    return fspec_fetch(h, index, op.spec.bins, applications, op.rule.e, out, words, reset != 0);
}

int fusion_spectrum_clear(fpic_handle* h)
{
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum_clear")) return rc;
    h->es->diag.fspec_ops.clear();   // (applications in flight keep their slots; a later registration zeroes its own in stream order)
    return FPIC_OK;
}

// the hook's part (diag_after_substep, after the fusion tallies): every registered spectrum that is due, in registration order
static int fspec_after_substep(fpic_handle* h, uint64_t substep)
{
    Diag& g = h->es->diag;
    for (size_t k = 0; k < g.fspec_ops.size(); ++k) {
        FspecOp& op = g.fspec_ops[k];
        if (substep % static_cast<uint64_t>(op.every)) continue;
        op.applications++;
        fesfusion::Rule r = op.rule;
        r.epoch = static_cast<uint32_t>(substep + op.spec.tally.epoch);
        if (int rc = fspec_apply(h, op.spec.tally, r, op.axis, static_cast<int>(k), false)) return rc;
    }
    return FPIC_OK;
}
