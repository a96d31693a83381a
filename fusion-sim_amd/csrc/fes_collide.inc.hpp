// fes_collide.inc.hpp: the Monte Carlo collision operator of a CART3D handle (fpic_collide, fpic_collide_register,
// fpic_collide_stats, fpic_collide_clear) — part of fes_api.hip's translation unit (included there after fes_load.inc.hpp,
// inside namespace fes).  The rule and the checks of a request are fes_collide_core.hpp, the passes fes_collide_kernels.hpp.
//
// EXCHANGE and ELASTIC have two hand-outs of their candidates, chosen by P_max = K 2^-32 (collide_compacts): the wave-shared
// loop, and between 2^-8 and 2^-3 the queue in LDS (DESIGN 4.16 has the measurements behind the two thresholds).
// One launch per application over the range of pass_head (fes_ops.inc.hpp).  The counts go to the family's rows
// (fes_ops.inc.hpp): four words per row.  A registered operator is enqueued by the hook with no host synchronisation and no
// collective; fpic_collide_stats reads its row.

constexpr int kCollideWords = 4;                         // per operator: (unused), candidates, collided, clipped
constexpr int kCollideNow = FPIC_COLLIDE_MAX_OPS;        // the row of fpic_collide

static int collide_room(fpic_handle* h) { return h->es->diag.collide.rows.room(h, kCollideWords, FPIC_COLLIDE_MAX_OPS + 1); }

// the instance of KIND for the request's form (null-collision test or not) and hand-out (collide_compacts)
template <typename T, int KIND>
static void collide_launch(fpic_handle* h, const CollideArgs<T>& a, unsigned grid)
{
    const bool compact = collide_compacts(a.r.K);
    if (a.r.nullc) {
        if (compact) collide_kernel<T, KIND, true, true><<<grid, kCollideThreads, 0, h->stream>>>(a);
        else collide_kernel<T, KIND, true, false><<<grid, kCollideThreads, 0, h->stream>>>(a);
    } else {
        if (compact) collide_kernel<T, KIND, false, true><<<grid, kCollideThreads, 0, h->stream>>>(a);
        else collide_kernel<T, KIND, false, false><<<grid, kCollideThreads, 0, h->stream>>>(a);
    }
}

// one application of `r` to species `sp`, its counts added to words[1 .. 4): enqueued, nothing waited for
template <typename T>
static int collide_enqueue(fpic_handle* h, const Species& sp, const fescoll::Rule& r, unsigned long long* words)
{
    const bool relax = r.kind == FPIC_COLLIDE_RELAX;
    CollideArgs<T> a{};
    const unsigned grid = pass_head(h, sp, kCollideBlocks, a);
    if (!grid || (!relax && r.K == 0)) return FPIC_OK;   // (nothing can collide: nothing is launched)
    a.counts = words + 1;
    a.r = r;
    if (relax) relax_kernel<T><<<grid, kCollideThreads, 0, h->stream>>>(a);
    else if (r.kind == FPIC_COLLIDE_EXCHANGE) collide_launch<T, FPIC_COLLIDE_EXCHANGE>(h, a, grid);
    else collide_launch<T, FPIC_COLLIDE_ELASTIC>(h, a, grid);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int collide_apply(fpic_handle* h, const fpic_collide_spec& spec, uint32_t epoch, unsigned long long* words)
{
    const Species& sp = h->es->sp[spec.species];
    const fescoll::Rule r = fescoll::rule_of(spec, epoch);
    return h->prec == FPIC_F32 ? collide_enqueue<float>(h, sp, r, words) : collide_enqueue<double>(h, sp, r, words);
}

static void collide_result(fpic_collide_result* out, uint64_t applications, const uint64_t* got)
{
    out->applications = applications;
    out->candidates = got[1];
    out->collided = got[2];
    out->clipped = got[3];
}

int collide(fpic_handle* h, const fpic_collide_spec* spec, fpic_collide_result* out)
{
    State* st = h->es;
    const OpRows& rows = st->diag.collide.rows;
    if (const char* why = fescoll::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_collide_result{};
    const fescoll::Rule r = fescoll::rule_of(*spec, spec->epoch);
    if (spec->kind != FPIC_COLLIDE_RELAX && r.K == 0) return FPIC_OK;
    if (int rc = collide_room(h)) return rc;
    if (int rc = rows.zero(h, kCollideNow)) return rc;
    if (int rc = collide_apply(h, *spec, spec->epoch, rows.row(kCollideNow))) return rc;
    uint64_t got[kCollideWords] = {};
    if (int rc = rows.fetch(h, kCollideNow, got)) return rc;
    if (out) collide_result(out, 1, got);
    return FPIC_OK;
}

int collide_register(fpic_handle* h, const fpic_collide_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.collide;
    if (const char* why = fescoll::check(spec, static_cast<int>(h->es->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = ops_check_register(h, f, fesops::kCollide, every)) return rc;
    if (int rc = collide_room(h)) return rc;
    if (int rc = f.rows.zero(h, f.ops.size())) return rc;
    CollideOp op;
    op.spec = *spec;
    return ops_push(f, op, every, index);
}

int collide_stats(fpic_handle* h, int index, int scope, fpic_collide_result* out)
{
    auto& f = h->es->diag.collide;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kCollide, index, scope, out, collective)) return rc;
    uint64_t got[kCollideWords] = {};
    if (int rc = f.rows.fetch(h, index, got)) return rc;
    if (collective)
        if (int rc = diag_sum_ranks(h, got, kCollideWords)) return rc;
    collide_result(out, f.ops[index].applications, got);   // (applications: the same on every rank, not summed)
    return FPIC_OK;
}

int collide_clear(fpic_handle* h) { return ops_clear(h->es->diag.collide); }

// the hook's part: every registered operator that is due, at the epoch of the sub-step
static int collide_after_substep(fpic_handle* h, uint64_t substep)
{
    auto& f = h->es->diag.collide;
    return ops_run_due<true>(f, OpsEvery{ substep }, [&](CollideOp& op, size_t k) { return collide_apply(h, op.spec, static_cast<uint32_t>(substep + op.spec.epoch), f.rows.row(k)); });
}
