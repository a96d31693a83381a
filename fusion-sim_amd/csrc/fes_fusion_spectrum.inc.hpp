// fes_fusion_spectrum.inc.hpp: the fusion product spectra of a CART3D handle (fpic_fusion_spectrum,
// fpic_fusion_spectrum_register, fpic_fusion_spectrum_read, fpic_fusion_spectrum_clear) — part of fes_api.hip's translation
// unit (included there after fes_fusion.inc.hpp, inside namespace fes).  The rule and the checks of a request are
// fes_fusion_spectrum_core.hpp on top of fes_fusion_core.hpp, the pass fes_fusion_spectrum_kernels.hpp.
//
// One application: per species of the request fpic_pair's cell index (pair_index<T>, into the Diag's index buffers,
// unchanged), then the spectrum pass — all enqueued on the handle's stream, nothing read back.  The family's rows
// (fes_ops.inc.hpp) hold the tally's eight count words and a table each (the tables an allocation of their own); the
// histogram words are rows of their own beside them (Diag::fspec_bins).  A table is uploaded at the call or at the
// registration (which waits for the copy); the hook never allocates, never waits and never reads back.
// A handle with a Domain is refused as fpic_fusion refuses it.

constexpr int kFspecNow = FPIC_FUSION_SPECTRUM_MAX_OPS;      // the row of fpic_fusion_spectrum
constexpr size_t kFspecSlotWords = static_cast<size_t>(kFspecEntriesMax) * 2;

// the row starts from zero with the request's table, in stream order; returns after the table has been copied
static int fspec_begin(fpic_handle* h, int slot, const fpic_fusion_spec& tally)
{
    Diag& g = h->es->diag;
    OpRows& rows = g.fspec.rows;
    if (int rc = rows.room(h, kFusionWords, FPIC_FUSION_SPECTRUM_MAX_OPS + 1, FPIC_FUSION_TABLE_MAX, true)) return rc;
    if (int rc = g.fspec_bins.room(h, static_cast<int>(kFspecSlotWords), FPIC_FUSION_SPECTRUM_MAX_OPS + 1)) return rc;
    if (int rc = rows.zero(h, slot)) return rc;
    if (int rc = g.fspec_bins.zero(h, slot)) return rc;
    HIP_TRY(h, hipMemcpyAsync(rows.table(slot), tally.sigma, static_cast<size_t>(tally.n) * sizeof(double), hipMemcpyHostToDevice, h->stream));
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
    const unsigned grid = pair_head(st, sa, sb, a);
    a.counts = g.fspec.rows.row(slot);
    a.words = g.fspec_bins.row(slot);
    a.table = g.fspec.rows.table(slot);
    a.r = r;
    a.s = s;
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

// the row's counts and bins -> out, words ((bins + 2) x 2, every entry joined); waits for the copies
static int fspec_fetch(fpic_handle* h, int slot, int bins, uint64_t applications, int e, fpic_fusion_result* out, uint64_t* words, bool reset)
{
    Diag& g = h->es->diag;
    uint64_t got[kFusionWords] = {};
    const size_t nwords = static_cast<size_t>(bins + 2) * 2;
    if (int rc = g.fspec.rows.copy(h, slot, got, kFusionWords)) return rc;
    if (words)
        if (int rc = g.fspec_bins.copy(h, slot, words, nwords)) return rc;
    if (reset) {   // (behind the copies, in stream order)
        if (int rc = g.fspec.rows.zero(h, slot)) return rc;
        if (int rc = g.fspec_bins.zero(h, slot)) return rc;
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
    auto& f = st->diag.fspec;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum_register")) return rc;
    if (int rc = fspec_check(h, spec)) return rc;
    if (int rc = ops_check_register(h, f, fesops::kFspec, every)) return rc;
    if (int rc = fusion_buffers(h, spec->tally, true)) return rc;   // (sized now: the hook finds them in place and never grows them)
    if (int rc = fspec_begin(h, static_cast<int>(f.ops.size()), spec->tally)) return rc;
    FspecOp op;
    op.spec = *spec;
    op.spec.tally.sigma = nullptr;  // (the table is on the device; the caller's need not outlive this call)
    op.rule = fesfusion::rule_of(spec->tally, spec->tally.epoch, st->W, fusion_dv(st));
    op.axis = fspec_rule(st, *spec);
    return ops_push(f, op, every, index);
}

int fusion_spectrum_read(fpic_handle* h, int index, fpic_fusion_result* out, uint64_t* words, int reset)
{
    auto& f = h->es->diag.fspec;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum_read")) return rc;
    if (int rc = ops_check_index(h, f, fesops::kFspec, index)) return rc;
    if (!out && !words && !reset) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    FspecOp& op = f.ops[index];
    const uint64_t applications = op.applications;
    if (reset) op.applications = 0;
    return fspec_fetch(h, index, op.spec.bins, applications, op.rule.e, out, words, reset != 0);
}

int fusion_spectrum_clear(fpic_handle* h)
{
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_spectrum_clear")) return rc;
    return ops_clear(h->es->diag.fspec);
}

// the hook's part: every registered spectrum that is due — the registered rules at the epoch of the sub-step
static int fspec_after_substep(fpic_handle* h, uint64_t substep)
{
    return ops_run_due<true>(h->es->diag.fspec, OpsEvery{ substep }, [&](FspecOp& op, size_t k) {
        fesfusion::Rule r = op.rule;
        r.epoch = static_cast<uint32_t>(substep + op.spec.tally.epoch);
        return fspec_apply(h, op.spec.tally, r, op.axis, static_cast<int>(k), false);
    });
}
