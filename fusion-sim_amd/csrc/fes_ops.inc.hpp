// fes_ops.inc.hpp: what the registered operators of a CART3D handle share — part of fes_api.hip's translation
// unit (included there before fes_collide.inc.hpp, inside namespace fes).  The types are in fes_state.inc.hpp (OpRows, OpCommon,
// OpFamily, the list FES_OP_FAMILIES), the checks and the families' messages in fes_ops_core.hpp.
//
// Every family (collide, force, gas, pair, fusion, fusion_spectrum, remove, inject, ionize, burn) has a call that applies a request now and
// calls that register it, read its totals and drop the registrations.  Here are the parts that do not depend on the family: the
// rows (allocation, a row's place, zeroing, the copy back), the registration's checks and its tail, the head of a stats read,
// the loop of the sub-step hook over the operators that are due, and the question whether anything is registered at all.  A
// family keeps its request's checks, when an operator is due, its launch, and what a row's words mean.

inline int OpRows::room(fpic_handle* h, int words_per_row, size_t nrows, size_t tab_doubles, bool tab_apart)
{
    const size_t word_bytes = nrows * words_per_row * sizeof(unsigned long long), tab_bytes = nrows * tab_doubles * sizeof(double);
    void* p = nullptr;
    if (!dev) {
        if (int rc = dev_alloc(h, &p, tab_apart ? word_bytes : word_bytes + tab_bytes, &h->bytes_grid)) return rc;
        dev = static_cast<unsigned long long*>(p);
        words = words_per_row;
        rows = nrows;
        tab = tab_doubles;
        apart = tab_apart;
        if (!tab_apart) tab_dev = reinterpret_cast<double*>(static_cast<unsigned char*>(p) + word_bytes);
        HIP_TRY(h, hipMemsetAsync(dev, 0, word_bytes, h->stream));
    }
    if (tab_apart && !tab_dev) {
        if (int rc = dev_alloc(h, &p, tab_bytes, &h->bytes_grid)) return rc;
        tab_dev = static_cast<double*>(p);
    }
    return FPIC_OK;
}
inline int OpRows::zero(fpic_handle* h, size_t k, size_t n) const
{
    HIP_TRY(h, hipMemsetAsync(row(k), 0, n * words * sizeof(unsigned long long), h->stream));
    return FPIC_OK;
}
inline int OpRows::copy(fpic_handle* h, size_t k, uint64_t* got, size_t nwords) const
{
    HIP_TRY(h, hipMemcpyAsync(got, row(k), nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    return FPIC_OK;
}
inline int OpRows::fetch(fpic_handle* h, size_t k, uint64_t* got) const
{
    if (int rc = copy(h, k, got, words)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}
inline void OpRows::release()
{
    if (dev) (void)hipFree(dev);
    if (apart && tab_dev) (void)hipFree(tab_dev);
    *this = OpRows();
}

// a registration after the family's own refusals: the period (a family without one passes 1) and the room
// (the forms that take the messages themselves serve a family that keeps its own beside the shared table)
template <typename Op>
static int ops_check_register(fpic_handle* h, const OpFamily<Op>& f, const fesops::Messages& m, int every)
{
    if (const char* why = fesops::check_register(every, static_cast<int>(f.ops.size()), m.max, m.full)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    return FPIC_OK;
}
template <typename Op>
static int ops_check_register(fpic_handle* h, const OpFamily<Op>& f, int family, int every)
{
    return ops_check_register(h, f, fesops::messages(family), every);
}
// the tail of a registration: the operator behind the others with nothing applied yet, its place (the row the family has
// prepared for it) to the caller
template <typename Op>
static int ops_push(OpFamily<Op>& f, Op op, int every, int* index)
{
    const int at = static_cast<int>(f.ops.size());
    op.every = every;
    op.applications = 0;
    f.ops.push_back(std::move(op));
    if (index) *index = at;
    return FPIC_OK;
}
template <typename Op>
static int ops_check_index(fpic_handle* h, const OpFamily<Op>& f, const fesops::Messages& m, int index)
{
    if (const char* why = fesops::check_index(index, static_cast<int>(f.ops.size()), m.index)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    return FPIC_OK;
}
template <typename Op>
static int ops_check_index(fpic_handle* h, const OpFamily<Op>& f, int family, int index)
{
    return ops_check_index(h, f, fesops::messages(family), index);
}
// the head of a stats read after the family's own refusals: `out`, then the index, then the scope
template <typename Op>
static int ops_stats_head(fpic_handle* h, const OpFamily<Op>& f, const fesops::Messages& m, int index, int scope, const void* out, bool& collective)
{
    if (!out) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    if (int rc = ops_check_index(h, f, m, index)) return rc;
    return diag_scope(h, scope, collective);
}
template <typename Op>
static int ops_stats_head(fpic_handle* h, const OpFamily<Op>& f, int family, int index, int scope, const void* out, bool& collective)
{
    return ops_stats_head(h, f, fesops::messages(family), index, scope, out, collective);
}
// (applications in flight keep their rows and tables; a later registration rewrites its own in stream order)
template <typename Op>
static int ops_clear(OpFamily<Op>& f)
{
    f.ops.clear();
    return FPIC_OK;
}

// the hook's loop over a family: every operator that is due(op), in registration order, apply(op, k) with k its row.
// COUNT_FIRST: the application is counted before it is enqueued (the passes that nothing waits for), else after it has
// succeeded (the sinks and sources, whose applications can refuse).  Stops at the first failure
template <bool COUNT_FIRST, typename Op, typename Due, typename Apply>
static int ops_run_due(OpFamily<Op>& f, Due due, Apply apply)
{
    for (size_t k = 0; k < f.ops.size(); ++k) {
        Op& op = f.ops[k];
        if (!due(op)) continue;
        if (COUNT_FIRST) op.applications++;
        if (int rc = apply(op, k)) return rc;
        if (!COUNT_FIRST) op.applications++;
    }
    return FPIC_OK;
}
// due every op.every-th sub-step
struct OpsEvery {
    uint64_t substep;
    bool operator()(const OpCommon& op) const { return substep % static_cast<uint64_t>(op.every) == 0; }
};

// the head of a pass's arguments (fes_pass.hpp): the slots [0, n) of `sp` and, while a migration rides on the next push, the
// arrivals behind them (they follow at tail_first = n: one range, as the flat pass of mom_enqueue).  Returns the pass's grid,
// at most `blocks` workgroups of kPassThreads lanes with a group of four slots each; 0: no slot, nothing to launch
template <typename T>
static unsigned pass_head(const fpic_handle* h, const Species& sp, int blocks, PassArgs<T>& a)
{
    a.slab = static_cast<T*>(sp.slab[sp.cur]);
    a.id = sp.ids_identity ? nullptr : sp.id[sp.cur];
    a.n_pad = sp.n_pad;
    a.s1 = std::min(sp.n + sp.tail_count, sp.n_pad);
    a.dead = h->es->dom ? 1 : 0;
    const size_t groups = (a.s1 + 3) / 4;
    return static_cast<unsigned>(std::min<size_t>(blocks, (groups + kPassThreads - 1) / kPassThreads));
}

static bool ops_registered(const Diag& g)
{
#define X(f) || !g.f.ops.empty()
    return false FES_OP_FAMILIES_ALL(X);
#undef X
}
