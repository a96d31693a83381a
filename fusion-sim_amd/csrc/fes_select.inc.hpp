// fes_select.inc.hpp: the particle selection of a CART3D handle (fpic_select) — part of fes_api.hip's translation unit
// (included there after fes_hist.inc.hpp, inside namespace fes).  The rule and the checks of a request are
// fes_select_core.hpp, the pass fes_select_kernels.hpp.
//
// A call zeroes the cursor on the handle's stream, launches one pass over the species' slots (the count query, or the
// delivering pass into a device buffer of min(capacity, n) rows), copies the cursor back and, if the rows fit, the rows; it
// sorts a permutation by id on the host, casts and writes the caller's arrays.  GLOBAL on a rank with a communicator sums
// the ranks' counts (diag_sum_ranks), gathers them and then the rows in chunks of kSelectGatherRows padded to the largest
// count (diag_gather, fes_record.inc.hpp); every rank merges the same rows in ascending id.

constexpr size_t kSelectGatherRows = size_t(1) << 15;   // 0.9 MiB (fp32) / 1.7 MiB (fp64) per rank and chunk

// the device buffer: the cursor (16 bytes), out_id[rows] (padded to 16 bytes), out_state[6][rows]
static size_t select_state_offset(size_t rows) { return 16 + (rows * sizeof(uint32_t) + 15) / 16 * 16; }

static int select_buffer(fpic_handle* h, size_t bytes)
{
    Diag& g = h->es->diag;
    if (g.sel_bytes >= bytes) return FPIC_OK;
    if (g.sel) { // (grows to the largest request)
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipFree(g.sel));
        h->bytes_grid -= g.sel_bytes;
        g.sel = nullptr;
        g.sel_bytes = 0;
    }
    if (int rc = dev_alloc(h, &g.sel, bytes, &h->bytes_grid)) return rc;
    g.sel_bytes = bytes;
    return FPIC_OK;
}

// rows of a selection on the host as the pass leaves them: id[m], st[6][m], in no particular order
template <typename T>
struct SelectRows {
    size_t m = 0;
    std::vector<uint32_t> id;
    std::vector<T> st;
};

template <typename T, int NA>
static void select_launch(fpic_handle* h, const SelectArgs<T>& a, bool deliver, unsigned long long* cursor)
{
    if (deliver) select_kernel<T, NA, true><<<kSelectBlocks, kSelectThreads, 0, h->stream>>>(a, cursor);
    else select_kernel<T, NA, false><<<kSelectBlocks, kSelectThreads, 0, h->stream>>>(a, cursor);
}

// the pass of one request over this handle's slots: `matched`, and the rows if they fit `capacity`
template <typename T>
static int select_local(fpic_handle* h, const fpic_select_spec& spec, uint64_t capacity, uint64_t& matched, SelectRows<T>& rows)
{
    State* st = h->es;
    const Species& sp = st->sp[spec.species];
    const size_t cap = static_cast<size_t>(std::min<uint64_t>(capacity, sp.n));
    const size_t off = select_state_offset(cap);
    if (int rc = select_buffer(h, off + 6 * cap * sizeof(T))) return rc;
    unsigned char* dev = static_cast<unsigned char*>(st->diag.sel);
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(dev);
    HIP_TRY(h, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), h->stream));
    matched = 0;
    rows.m = 0;
    if (!sp.n) return FPIC_OK; // (nothing is read)
    SelectArgs<T> a{};
    a.slab = static_cast<const T*>(sp.slab[sp.cur]);
    a.id = sp.id[sp.cur];
    a.n = sp.n;
    a.n_pad = sp.n_pad;
    a.dead = st->dom ? 1 : 0;
    // the arrays the pass streams, in slab order: those the terms name, and x for the dead test
    const uint32_t arrays = fessel::arrays_of(spec) | (a.dead ? 1u : 0u);
    int na = 0, at[6] = {};
    for (int c = 0; c < 6; ++c)
        if (arrays >> c & 1u) {
            at[c] = na;
            a.src[na++] = a.slab + c * sp.n_pad;
        }
    for (int t = 0; t < spec.nterms; ++t) {
        if (spec.axis[t] == FPIC_AXIS_V2) {
            a.v2 = 1;
            a.v2_lo = spec.lo[t];
            a.v2_hi = spec.hi[t];
        } else {
            const int k = at[spec.axis[t]];
            a.term |= 1u << k;
            a.lo[k] = spec.lo[t];
            a.hi[k] = spec.hi[t];
        }
    }
    a.id_mod = spec.id_mod;
    a.id_rem = spec.id_rem;
    a.cap = cap;
    a.out_id = reinterpret_cast<uint32_t*>(dev + 16);
    a.out_state = reinterpret_cast<T*>(dev + off);
    const bool deliver = cap > 0;
    switch (na) {
    case 0: select_launch<T, 0>(h, a, deliver, cursor); break;
    case 1: select_launch<T, 1>(h, a, deliver, cursor); break;
    case 2: select_launch<T, 2>(h, a, deliver, cursor); break;
    case 3: select_launch<T, 3>(h, a, deliver, cursor); break;
    case 4: select_launch<T, 4>(h, a, deliver, cursor); break;
    case 5: select_launch<T, 5>(h, a, deliver, cursor); break;
    default: select_launch<T, 6>(h, a, deliver, cursor); break;
    }
    HIP_TRY(h, hipGetLastError());
    unsigned long long got = 0;
    HIP_TRY(h, hipMemcpyAsync(&got, cursor, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    matched = got;
    if (!got || got > capacity) return FPIC_OK;
    const size_t m = static_cast<size_t>(got);   // (<= cap: a species matches at most its n slots)
    rows.m = m;
    rows.id.resize(m);
    rows.st.resize(6 * m);
    HIP_TRY(h, hipMemcpyAsync(rows.id.data(), a.out_id, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    for (int c = 0; c < 6; ++c) HIP_TRY(h, hipMemcpyAsync(rows.st.data() + c * m, a.out_state + c * cap, m * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

// the ranks' rows -> `rows` of every rank: counts[r] rows of rank r, in rank order
template <typename T>
static int select_gather_rows(fpic_handle* h, const uint64_t* counts, SelectRows<T>& rows)
{
    const int world = h->comm->world, rank = h->comm->rank;
    size_t total = 0, most = 0;
    std::vector<size_t> first(world);
    for (int r = 0; r < world; ++r) {
        first[r] = total;
        total += static_cast<size_t>(counts[r]);
        most = std::max(most, static_cast<size_t>(counts[r]));
    }
    SelectRows<T> all;
    all.m = total;
    all.id.resize(total);
    all.st.resize(6 * total);
    std::vector<unsigned char> block, gathered;
    for (size_t at = 0; at < most; at += kSelectGatherRows) {
        const size_t m = std::min(kSelectGatherRows, most - at);
        const size_t state_at = (m * sizeof(uint32_t) + 7) / 8 * 8, bytes = state_at + 6 * m * sizeof(T);   // (a multiple of 8)
        auto held = [&](int r) { return at < counts[r] ? std::min(m, static_cast<size_t>(counts[r]) - at) : size_t(0); };
        block.assign(bytes, 0);
        if (const size_t k = held(rank)) {
            std::memcpy(block.data(), rows.id.data() + at, k * sizeof(uint32_t));
            for (int c = 0; c < 6; ++c) std::memcpy(block.data() + state_at + c * m * sizeof(T), rows.st.data() + c * rows.m + at, k * sizeof(T));
        }
        if (int rc = diag_gather(h, block.data(), bytes, gathered)) return rc;
        for (int r = 0; r < world; ++r) {
            const size_t k = held(r);
            if (!k) continue;
            const unsigned char* from = gathered.data() + static_cast<size_t>(r) * bytes;
            std::memcpy(all.id.data() + first[r] + at, from, k * sizeof(uint32_t));
            for (int c = 0; c < 6; ++c) std::memcpy(all.st.data() + c * total + first[r] + at, from + state_at + c * m * sizeof(T), k * sizeof(T));
        }
    }
    rows = std::move(all);
    return FPIC_OK;
}

// the rows in ascending id into the caller's arrays, the stored values cast to Out
template <typename T, typename Out>
static void select_write(const SelectRows<T>& rows, uint32_t* ids, Out* pos, Out* vel)
{
    const size_t m = rows.m;
    std::vector<uint32_t> perm(m);
    for (size_t k = 0; k < m; ++k) perm[k] = static_cast<uint32_t>(k);
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return rows.id[a] != rows.id[b] ? rows.id[a] < rows.id[b] : a < b; });
    for (size_t r = 0; r < m; ++r) {
        const size_t s = perm[r];
        if (ids) ids[r] = rows.id[s];
        for (int c = 0; c < 3; ++c) {
            if (pos) pos[3 * r + c] = static_cast<Out>(rows.st[c * m + s]);
            if (vel) vel[3 * r + c] = static_cast<Out>(rows.st[(3 + c) * m + s]);
        }
    }
}

template <typename T>
static int select_run(fpic_handle* h, const fpic_select_spec& spec, bool collective, uint64_t capacity, uint32_t* ids, void* pos, void* vel, int dtype, uint64_t* matched)
{
    SelectRows<T> rows;
    uint64_t mine = 0;
    if (int rc = select_local<T>(h, spec, capacity, mine, rows)) return rc;
    *matched = mine;
    if (collective) {
        std::vector<unsigned char> all;
        if (int rc = diag_gather(h, &mine, sizeof(mine), all)) return rc;
        std::vector<uint64_t> counts(h->comm->world);
        std::memcpy(counts.data(), all.data(), counts.size() * sizeof(uint64_t));
        uint64_t total = mine;
        if (int rc = diag_sum_ranks(h, &total, 1)) return rc;
        *matched = total;
        if (total > capacity) return FPIC_OK;   // (the same on every rank: nobody enters the gather of the rows)
        if (int rc = select_gather_rows<T>(h, counts.data(), rows)) return rc;
    }
    if (*matched > capacity) return FPIC_OK;
    if (dtype == FPIC_F32) select_write<T, float>(rows, ids, static_cast<float*>(pos), static_cast<float*>(vel));
    else select_write<T, double>(rows, ids, static_cast<double*>(pos), static_cast<double*>(vel));
    return FPIC_OK;
}

int select(fpic_handle* h, const fpic_select_spec* spec, int scope, uint64_t capacity, uint32_t* ids, void* pos_aos, void* vel_aos, int dtype, uint64_t* matched)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    if (!matched) return fail(h, FPIC_ERR_INVALID_ARG, ".matched <- Non-optional property is undefined!");
    if (const char* why = fessel::check(*spec, static_cast<int>(h->es->sp.size()), capacity, ids || pos_aos || vel_aos, dtype)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    return h->prec == FPIC_F32 ? select_run<float>(h, *spec, collective, capacity, ids, pos_aos, vel_aos, dtype, matched)
                               : select_run<double>(h, *spec, collective, capacity, ids, pos_aos, vel_aos, dtype, matched);
}
