// fes_record.inc.hpp: what the diagnostics of a CART3D handle share — part of fes_api.hip's translation unit (included there
// before fes_diag.inc.hpp, inside namespace fes): the scope of a call, the ranks' gather and their integer sum, and the
// recorder (Recorder, fes_state.inc.hpp) behind fpic_energy_record / fpic_series_record / fpic_modes_record and their
// histories.  The ring's arithmetic and the ranks' agreement are fes_diag_core.hpp.
//
// A recorder's owner builds its request and says what a row holds (its enqueue) and how rows reach the caller (its
// delivery); arming, the due slot, the drain and a single row now are here, once.

constexpr size_t kHistGatherWords = size_t(1) << 17;   // 1 MiB per rank and chunk of a sum over the ranks

// whether a call of `scope` is collective: GLOBAL on a rank of a decomposition over more than one handle
static int diag_scope(fpic_handle* h, int scope, bool& collective)
{
    if (scope != FPIC_DIAG_LOCAL && scope != FPIC_DIAG_GLOBAL) return fail(h, FPIC_ERR_INVALID_ARG, ".scope <- must be 0 (local) or 1 (global)");
    const Domain* d = h->es->dom;
    collective = scope == FPIC_DIAG_GLOBAL && d && d->world > 1;
    if (!collective) return FPIC_OK;
    if (!h->comm)
        return fail(h, FPIC_ERR_STATE, "GLOBAL on a member of an in-process group: add up the members' LOCAL values (BoxGroup.energy)");
    if (h->comm->world != d->world || h->comm->rank != d->rank)
        return fail(h, FPIC_ERR_STATE, "the communicator (rank %d of %d) and the decomposition (rank %d of %d) disagree", h->comm->rank, h->comm->world, d->rank, d->world);
    return FPIC_OK;
}

// `bytes` (a multiple of 8) of every rank, in rank order, into `all`: one in-place ncclAllGather on the handle's stream
static int diag_gather(fpic_handle* h, const void* mine, size_t bytes, std::vector<unsigned char>& all)
{
    Diag& g = h->es->diag;
    const int world = h->comm->world, rank = h->comm->rank;
    const size_t need = bytes * world;
    if (g.gather_bytes < need) {
        if (g.gather) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, hipFree(g.gather));
            h->bytes_grid -= g.gather_bytes;
            g.gather = nullptr;
            g.gather_bytes = 0;
        }
        if (int rc = dev_alloc(h, &g.gather, need, &h->bytes_grid)) return rc;
        g.gather_bytes = need;
    }
    unsigned char* buf = static_cast<unsigned char*>(g.gather);
    HIP_TRY(h, hipMemcpyAsync(buf + rank * bytes, mine, bytes, hipMemcpyHostToDevice, h->stream));
    if (int e = fcomm::check(h, fdyn::rccl().AllGather(buf + rank * bytes, buf, bytes / sizeof(double), ncclDouble, h->comm->nccl, h->stream), "ncclAllGather")) return e;
    all.resize(need);
    HIP_TRY(h, hipMemcpyAsync(all.data(), buf, need, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

// words[0 .. n) of this rank -> their sums over the ranks, in place: gathered in chunks of kHistGatherWords, added as integers
// in rank order (fesdiag::add_words), so every rank gets the same sums
static int diag_sum_ranks(fpic_handle* h, uint64_t* words, size_t n)
{
    std::vector<unsigned char> all;
    for (size_t at = 0; at < n; at += kHistGatherWords) {
        const size_t m = std::min(kHistGatherWords, n - at);
        if (int rc = diag_gather(h, words + at, m * sizeof(uint64_t), all)) return rc;
        fesdiag::add_words(reinterpret_cast<const uint64_t*>(all.data()), m, h->comm->world, words + at);
    }
    return FPIC_OK;
}

// ---------------------------------------------------------------- the recorder

// the settings of a *_record call, checked before its owner builds the request
static int rec_check(fpic_handle* h, int every, uint32_t capacity)
{
    if (every < 0) return fail(h, FPIC_ERR_INVALID_ARG, ".every <- must be >= 0 (0 turns recording off)");
    if (every > 0 && capacity < 1) return fail(h, FPIC_ERR_INVALID_ARG, ".capacity <- must be at least 1");
    return FPIC_OK;
}

// recording off and the ring given back; `request_live`: the owner holds a request that rows in flight read, and frees it next
static int rec_disarm(fpic_handle* h, Recorder& r, bool request_live)
{
    if (r.dev || request_live) HIP_TRY(h, hipStreamSynchronize(h->stream)); // (recorded rows still in flight write to it)
    if (r.dev) {
        HIP_TRY(h, hipFree(r.dev));
        h->bytes_grid -= r.ring.cap * r.row_bytes;
    }
    r = Recorder();
    return FPIC_OK;
}

// a disarmed recorder takes a ring of `capacity` rows of `row_bytes` and records after every `every`-th sub-step; on a refusal
// it stays off (and the owner frees the request it made for it)
static int rec_arm(fpic_handle* h, Recorder& r, int every, uint32_t capacity, size_t row_bytes)
{
    if (int rc = dev_alloc(h, &r.dev, static_cast<size_t>(capacity) * row_bytes, &h->bytes_grid)) return rc;
    r.row_bytes = row_bytes;
    r.ring.cap = capacity;
    r.substep.assign(capacity, 0);
    r.every = every;
    return FPIC_OK;
}

// the hook's two halves: the row (device memory) the recorder writes after sub-step `substep`, or nullptr if none is due;
// and, once the owner has enqueued it, the row counted (a failed enqueue leaves the ring as it was)
static void* rec_due(const Recorder& r, uint64_t substep)
{
    if (!r.every || substep % static_cast<uint64_t>(r.every)) return nullptr;
    return static_cast<unsigned char*>(r.dev) + r.ring.slot(r.ring.seq) * r.row_bytes;
}
static void rec_commit(Recorder& r, uint64_t substep)
{
    r.substep[r.ring.slot(r.ring.seq)] = substep;
    r.ring.commit();
}

// what a drain hands its owner: the pending rows in sequence order (8-byte words, cnt rows of row_bytes), where they start
// in the sequence, how many older ones the ring dropped; `query`: the call only asked, *n and *dropped are answered
struct Drain {
    std::vector<double> rows;
    uint64_t first = 0, cnt = 0, drop = 0;
    bool collective = false, query = false;
};

// a *_history call up to delivery.  `query`: the caller passed no room for rows; `missing`: the name of an output the owner
// needs for any row and did not get, or nullptr.  Under a collective call the ranks agree on (cnt, drop) first (one small
// gather), so that a mismatch stops every rank here instead of leaving some in the gather of the rows
static int rec_drain(fpic_handle* h, const Recorder& r, int scope, bool query, uint64_t capacity, const char* missing, uint64_t* n, uint64_t* dropped, Drain& d)
{
    if (!n) return fail(h, FPIC_ERR_INVALID_ARG, ".n <- Non-optional property is undefined!");
    if (int rc = diag_scope(h, scope, d.collective)) return rc;
    if (r.dev) r.ring.pending(d.first, d.cnt, d.drop);
    d.query = query;
    if (query) { // nothing is drained
        *n = d.cnt;
        if (dropped) *dropped = d.drop;
        return FPIC_OK;
    }
    if (capacity < d.cnt) return fail(h, FPIC_ERR_INVALID_ARG, ".capacity <- %llu rows are pending, room for %llu", static_cast<unsigned long long>(d.cnt), static_cast<unsigned long long>(capacity));
    if (d.cnt && missing) return fail(h, FPIC_ERR_INVALID_ARG, ".%s <- Non-optional property is undefined!", missing);
    d.rows.resize(d.cnt * r.row_bytes / sizeof(double));
    unsigned char* to = reinterpret_cast<unsigned char*>(d.rows.data());
    uint64_t slot[2], len[2];
    const int nr = r.ring.runs(d.first, d.cnt, slot, len);
    for (int k = 0; k < nr; to += len[k] * r.row_bytes, ++k)
        HIP_TRY(h, hipMemcpyAsync(to, static_cast<const unsigned char*>(r.dev) + slot[k] * r.row_bytes, len[k] * r.row_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!d.collective) return FPIC_OK;
    const double mine_n[2] = { static_cast<double>(d.cnt), static_cast<double>(d.drop) };
    std::vector<unsigned char> all;
    if (int rc = diag_gather(h, mine_n, sizeof(mine_n), all)) return rc;
    const double* ns = reinterpret_cast<const double*>(all.data());
    const int other = fesdiag::disagreeing_rank(ns, h->comm->world, mine_n[0], mine_n[1]);
    if (other >= 0)
        return fail(h, FPIC_ERR_STATE, "the ranks hold different numbers of recorded rows (%llu here, %.0f on rank %d): record with the same settings on every rank",
                    static_cast<unsigned long long>(d.cnt), ns[2 * other], other);
    return FPIC_OK;
}

// ... and after the owner's delivery has succeeded: the sub-steps of the rows (if asked for), the counts, the rows drained
static void rec_drained(Recorder& r, const Drain& d, uint64_t* substeps, uint64_t* n, uint64_t* dropped)
{
    for (uint64_t i = 0; substeps && i < d.cnt; ++i) substeps[i] = r.substep[r.ring.slot(d.first + i)];
    r.ring.mark_drained();
    *n = d.cnt;
    if (dropped) *dropped = d.drop;
}

// one row of the state now, for a *_now call: a scratch row of row_bytes (not counted in bytes_grid), the owner's
// enqueue(row), the row read back into `mine` and the stream waited for
template <typename Enqueue>
static int rec_row_now(fpic_handle* h, size_t row_bytes, const char* what, Enqueue enqueue, std::vector<double>& mine)
{
    void* row = nullptr;
    int rc = dev_alloc(h, &row, row_bytes, nullptr);
    if (rc == FPIC_OK) rc = enqueue(row);
    if (rc == FPIC_OK) {
        mine.resize(row_bytes / sizeof(double));
        hipError_t e = hipMemcpyAsync(mine.data(), row, row_bytes, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, FPIC_ERR_HIP, "%s read-back failed: %s", what, hipGetErrorString(e));
    }
    if (row) (void)hipFree(row);
    return rc;
}
