// fes_collide.inc.hpp: the Monte Carlo collision operator of a CART3D handle (fpic_collide, fpic_collide_register,
// fpic_collide_stats, fpic_collide_clear) — part of fes_api.hip's translation unit (included there after fes_load.inc.hpp,
// inside namespace fes).  The rule and the checks of a request are fes_collide_core.hpp, the passes fes_collide_kernels.hpp.
//
// EXCHANGE and ELASTIC have two passes, chosen by P_max = K 2^-32 (collide_compacts): the plain one, and between 2^-8 and 2^-3
// the one that compacts a workgroup's candidates into LDS (DESIGN 4.16 has the measurements behind the two thresholds).
// One launch per application over the slots [0, n) and, while a migration rides on the next push, the arrivals behind them
// (they follow at tail_first = n: one range, as the flat pass of mom_enqueue).  The counts go to device words of the handle:
// four per registered operator and four for the call that is applied now.  A registered operator is enqueued by the hook
// diag_after_substep with no host synchronisation and no collective; fpic_collide_stats reads its words.

constexpr int kCollideWords = 4;                         // per operator: (unused), candidates, collided, clipped
constexpr int kCollideNow = FPIC_COLLIDE_MAX_OPS;        // the words of fpic_collide

static int collide_words(fpic_handle* h)
{
    Diag& g = h->es->diag;
    if (g.coll) return FPIC_OK;
    void* p = nullptr;
    const size_t bytes = static_cast<size_t>(FPIC_COLLIDE_MAX_OPS + 1) * kCollideWords * sizeof(unsigned long long);
    if (int rc = dev_alloc(h, &p, bytes, &h->bytes_grid)) return rc;
    g.coll = static_cast<unsigned long long*>(p);
    HIP_TRY(h, hipMemsetAsync(g.coll, 0, bytes, h->stream));
    return FPIC_OK;
}

// one application of `r` to species `sp`, its counts added to words[1 .. 4): enqueued, nothing waited for
template <typename T>
static int collide_enqueue(fpic_handle* h, const Species& sp, const fescoll::Rule& r, unsigned long long* words)
{
    const bool relax = r.kind == FPIC_COLLIDE_RELAX;
    const size_t slots = std::min(sp.n + sp.tail_count, sp.n_pad);   // (the arrivals of a riding migration follow at tail_first = n)
    if (!slots || (!relax && r.K == 0)) return FPIC_OK;   // (nothing can collide: nothing is launched)
    CollideArgs<T> a{};
    a.slab = static_cast<T*>(sp.slab[sp.cur]);
    a.id = sp.ids_identity ? nullptr : sp.id[sp.cur];
    a.n_pad = sp.n_pad;
    a.s1 = slots;
    a.dead = h->es->dom ? 1 : 0;
    a.counts = words + 1;
    a.r = r;
    const size_t groups = (slots + 3) / 4;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(kCollideBlocks, (groups + kCollideThreads - 1) / kCollideThreads));
    const bool compact = collide_compacts(r.K);
    if (relax) relax_kernel<T><<<grid, kCollideThreads, 0, h->stream>>>(a);
    else if (compact) {
        if (r.kind == FPIC_COLLIDE_EXCHANGE) {
            if (r.nullc) collide_compact_kernel<T, FPIC_COLLIDE_EXCHANGE, true><<<grid, kCollideThreads, 0, h->stream>>>(a);
            else collide_compact_kernel<T, FPIC_COLLIDE_EXCHANGE, false><<<grid, kCollideThreads, 0, h->stream>>>(a);
        } else {
            if (r.nullc) collide_compact_kernel<T, FPIC_COLLIDE_ELASTIC, true><<<grid, kCollideThreads, 0, h->stream>>>(a);
            else collide_compact_kernel<T, FPIC_COLLIDE_ELASTIC, false><<<grid, kCollideThreads, 0, h->stream>>>(a);
        }
    }
    else if (r.kind == FPIC_COLLIDE_EXCHANGE) {
        if (r.nullc) collide_kernel<T, FPIC_COLLIDE_EXCHANGE, true><<<grid, kCollideThreads, 0, h->stream>>>(a);
        else collide_kernel<T, FPIC_COLLIDE_EXCHANGE, false><<<grid, kCollideThreads, 0, h->stream>>>(a);
    } else {
        if (r.nullc) collide_kernel<T, FPIC_COLLIDE_ELASTIC, true><<<grid, kCollideThreads, 0, h->stream>>>(a);
        else collide_kernel<T, FPIC_COLLIDE_ELASTIC, false><<<grid, kCollideThreads, 0, h->stream>>>(a);
    }
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int collide_apply(fpic_handle* h, const fpic_collide_spec& spec, uint32_t epoch, unsigned long long* words)
{
    const Species& sp = h->es->sp[spec.species];
    const fescoll::Rule r = fescoll::rule_of(spec, epoch);
    return h->prec == FPIC_F32 ? collide_enqueue<float>(h, sp, r, words) : collide_enqueue<double>(h, sp, r, words);
}

int collide(fpic_handle* h, const fpic_collide_spec* spec, fpic_collide_result* out)
{
    State* st = h->es;
    if (const char* why = fescoll::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_collide_result{};
    const fescoll::Rule r = fescoll::rule_of(*spec, spec->epoch);
    if (spec->kind != FPIC_COLLIDE_RELAX && r.K == 0) return FPIC_OK;
    if (int rc = collide_words(h)) return rc;
    unsigned long long* words = st->diag.coll + kCollideNow * kCollideWords;
    HIP_TRY(h, hipMemsetAsync(words, 0, kCollideWords * sizeof(unsigned long long), h->stream));
    if (int rc = collide_apply(h, *spec, spec->epoch, words)) return rc;
    unsigned long long got[kCollideWords] = {};
    HIP_TRY(h, hipMemcpyAsync(got, words, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (out) {
        out->applications = 1;
        out->candidates = got[1];
        out->collided = got[2];
        out->clipped = got[3];
    }
    return FPIC_OK;
}

int collide_register(fpic_handle* h, const fpic_collide_spec* spec, int every, int* index)
{
    Diag& g = h->es->diag;
    if (const char* why = fescoll::check(spec, static_cast<int>(h->es->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (const char* why = fescoll::check_register(every, static_cast<int>(g.coll_ops.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = collide_words(h)) return rc;
    const int at = static_cast<int>(g.coll_ops.size());
    HIP_TRY(h, hipMemsetAsync(g.coll + at * kCollideWords, 0, kCollideWords * sizeof(unsigned long long), h->stream));
    g.coll_ops.push_back(CollideOp{ *spec, every, 0 });
    if (index) *index = at;
    return FPIC_OK;
}

int collide_stats(fpic_handle* h, int index, int scope, fpic_collide_result* out)
{
    Diag& g = h->es->diag;
    if (!out) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    if (const char* why = fescoll::check_index(index, static_cast<int>(g.coll_ops.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    uint64_t got[kCollideWords] = {};
    HIP_TRY(h, hipMemcpyAsync(got, g.coll + index * kCollideWords, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (collective)
        if (int rc = diag_sum_ranks(h, got, kCollideWords)) return rc;
    out->applications = g.coll_ops[index].applications;   // (the same on every rank: not summed)
    out->candidates = got[1];
    out->collided = got[2];
    out->clipped = got[3];
    return FPIC_OK;
}

int collide_clear(fpic_handle* h)
{
    h->es->diag.coll_ops.clear();   // (applications in flight keep their words; a later registration zeroes its own in stream order)
    return FPIC_OK;
}

// the hook's part (diag_after_substep, after the sub-step is counted): every registered operator that is due, in
// registration order; nothing registered: nothing is enqueued
static int collide_after_substep(fpic_handle* h, uint64_t substep)
{
    Diag& g = h->es->diag;
    for (size_t k = 0; k < g.coll_ops.size(); ++k) {
        CollideOp& op = g.coll_ops[k];
        if (substep % static_cast<uint64_t>(op.every)) continue;
        op.applications++;
        if (int rc = collide_apply(h, op.spec, static_cast<uint32_t>(substep + op.spec.epoch), g.coll + k * kCollideWords)) return rc;
    }
    return FPIC_OK;
}
