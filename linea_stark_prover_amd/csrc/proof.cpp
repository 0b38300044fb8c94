// The proof object across the boundary: the wire format
// and a field-by-field view that maps 1:1 onto p3_uni_stark::Proof<SC>
// ([EXT p3-uni-stark proof.rs], produced at bin/src/main.rs:80-86 and
// consumed by p3_uni_stark::verify at bin/src/main.rs:88-96):
//   Proof { commitments: { trace, quotient_chunks },
//           opened_values: { trace_local, trace_next, quotient_chunks },
//           opening_proof: FriProof { commit_phase_commits, query_proofs,
//                                     final_poly, pow_witness },
//           degree_bits }
// lsp_proof_get_view hands out flat, query-major arrays of Montgomery-form
// elements (the lsp_fr convention); lsp_proof_from_view and
// lsp_proof_deserialize rebuild a proof handle from them (e.g. a Proof<SC>
// produced elsewhere, for lsp_verify).  Everything here is host code and
// treats its input bytes as untrusted (tests/test_proof_view.py fuzzes it,
// tools/sanitize builds it under ASan/UBSan).
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "prove_internal.hpp"
#include "wire.hpp"

namespace lsp {

namespace {
struct Recycler {
    std::mutex mu;
    std::vector<std::vector<uint8_t>> wires;
    std::vector<std::vector<lsp_query>> queries;
    static constexpr size_t KEEP = 4;  // proofs' worth held at most
};
Recycler& recycler() {
    static Recycler* r = new Recycler();  // never destroyed: frees may run during exit
    return *r;
}
}  // namespace

// LSP_RECYCLE=0: plain frees and fresh allocations (same-box A/B; read per call)
static bool recycle_on() {
    const char* e = std::getenv("LSP_RECYCLE");
    return !(e && *e == '0');
}

void proof_release(lsp_proof* p) {
    if (!p) return;
    if (!recycle_on()) {
        delete p;
        return;
    }
    Recycler& r = recycler();
    {
        std::lock_guard<std::mutex> g(r.mu);
        if (r.wires.size() < Recycler::KEEP && p->wire.capacity() > 0) r.wires.push_back(std::move(p->wire));
        if (r.queries.size() < Recycler::KEEP && p->queries.capacity() > 0) r.queries.push_back(std::move(p->queries));
    }
    delete p;
}

std::vector<uint8_t> recycled_wire() {
    if (!recycle_on()) return {};
    Recycler& r = recycler();
    std::lock_guard<std::mutex> g(r.mu);
    if (r.wires.empty()) return {};
    std::vector<uint8_t> v = std::move(r.wires.back());
    r.wires.pop_back();
    return v;
}

std::vector<lsp_query> recycled_queries() {
    if (!recycle_on()) return {};
    Recycler& r = recycler();
    std::lock_guard<std::mutex> g(r.mu);
    if (r.queries.empty()) return {};
    std::vector<lsp_query> v = std::move(r.queries.back());
    r.queries.pop_back();
    return v;
}

// two committed matrices: "LSPPRF02"; a third, the preprocessed one: "LSPPRF03" 
std::vector<uint8_t> serialize(const lsp_proof& p, HostPool* pool, std::vector<uint8_t>* reuse) {
    const size_t nm = p.mats.size();
    LSP_REQUIRE(nm == 2 || nm == 3, LSP_E_STATE, "a proof holds two or three committed matrices");
    size_t nfr = 1 + p.roots.size() + p.final_poly.size(), nu32 = 4 + nm;
    for (const OpenedMat& m : p.mats) nfr += m.ys.size() + (m.root_on_wire ? 1 : 0);
    // byte offset of every query's record (queries are written independently)
    std::vector<size_t> qoff(p.queries.size() + 1);
    size_t qbytes = 0;
    for (size_t i = 0; i < p.queries.size(); ++i) {
        const auto& q = p.queries[i];
        size_t f = q.sib.size(), u = q.open.size() + q.sib.size();
        for (auto& o : q.open) f += o.row.size() + o.path.size();
        for (auto& fp : q.fpath) f += fp.size();
        qoff[i] = qbytes;
        qbytes += 32 * f + 4 * u;
    }
    const size_t head = 8 + 4 * nu32 + 32 * nfr;  // header + the fields before the queries
    std::vector<uint8_t> b;
    if (reuse) b.swap(*reuse);
    // every byte is written below, so a recycled buffer needs no clearing
    // (resize value-initialises only what it adds)
    b.resize(head + qbytes);
    std::memcpy(b.data(), nm == 3 ? "LSPPRF03" : "LSPPRF02", 8);
    Writer w{b.data() + 8};
    w.u32(p.log_h);
    w.u32(p.log_q);
    w.u32(p.mats[MAT_TRACE].width);
    w.u32((uint32_t)p.queries.size());
    w.u32((uint32_t)p.roots.size());
    w.u32((uint32_t)p.final_poly.size());
    for (size_t m = MAT_QUOTIENT + 1; m < nm; ++m) w.u32(p.mats[m].width);
    for (const OpenedMat& m : p.mats)
        if (m.root_on_wire) w.fr(m.root);
    for (const OpenedMat& m : p.mats) w.frs(m.ys);
    w.frs(p.roots);
    w.frs(p.final_poly);
    w.fr(p.pow_w);
    if (w.p != b.data() + head) throw LspError(LSP_E_STATE, "proof serialization size mismatch");
    auto write_query = [&](size_t i) {
        const auto& q = p.queries[i];
        Writer wq{b.data() + head + qoff[i]};
        for (auto& o : q.open) {
            wq.frs(o.row);
            wq.path(o.path);
        }
        for (size_t r = 0; r < q.sib.size(); ++r) {
            wq.fr(q.sib[r]);
            wq.path(q.fpath[r]);
        }
    };
    if (pool && p.queries.size() > 1)
        pool->parallel_for(p.queries.size(), write_query);
    else
        for (size_t i = 0; i < p.queries.size(); ++i) write_query(i);
    return b;
}

// Untrusted bytes: every count is range-checked before anything is sized by
// it, and the buffer must be consumed exactly.
lsp_proof* deserialize(const uint8_t* buf, size_t len) {
    const bool prep = buf && len >= 8 && std::memcmp(buf, "LSPPRF03", 8) == 0;
    if (!buf || len < 8 + 24 || (!prep && std::memcmp(buf, "LSPPRF02", 8) != 0))
        throw LspError(LSP_E_ARG, "not an LSPPRF02 or LSPPRF03 proof");
    Reader r{buf, len};
    r.off = 8;
    auto p = std::make_unique<lsp_proof>();
    p->log_h = r.u32();
    p->log_q = r.u32();
    const uint32_t w = r.u32(), nq = r.u32(), nr = r.u32(), nf = r.u32();
    // LSPPRF03: the preprocessed matrix's width, range-checked like the trace's
    // before anything is sized by it (Reader::frs refuses what the bytes cannot hold)
    const uint32_t wp = prep ? r.u32() : 0;
    if (prep && (r.bad || wp == 0 || wp > (1u << 20))) throw LspError(LSP_E_ARG, "proof header out of range");
    if (r.bad || p->log_h > 40 || p->log_q > 20 || w == 0 || w > (1u << 20) || nr > 64 || nq > (1u << 20) ||
        nf == 0 || nf > (1u << 20) || (nf & (nf - 1)) != 0)
        throw LspError(LSP_E_ARG, "proof header out of range");
    const uint32_t widths[] = {w, 1u << p->log_q, wp};
    size_t wsum = 0;
    for (size_t m = 0; m < (prep ? 3u : 2u); ++m) {
        p->mats.emplace_back(m, widths[m]);
        wsum += widths[m];
    }
    for (OpenedMat& m : p->mats)
        if (m.root_on_wire) m.root = r.fr();
    for (OpenedMat& m : p->mats) r.frs(m.ys, (uint64_t)m.npoints * m.width);
    r.frs(p->roots, nr);
    r.frs(p->final_poly, nf);
    p->pow_w = r.fr();
    if (r.bad || nq > (len - r.off) / (32 * wsum)) throw LspError(LSP_E_ARG, "malformed proof bytes");
    p->queries.resize(nq);
    for (auto& qq : p->queries) {
        qq.open.resize(p->mats.size());
        for (size_t m = 0; m < p->mats.size(); ++m) {
            r.frs(qq.open[m].row, p->mats[m].width);
            r.frs(qq.open[m].path, r.u32());
        }
        qq.sib.resize(nr);
        qq.fpath.resize(nr);
        for (uint32_t k = 0; k < nr && !r.bad; ++k) {
            qq.sib[k] = r.fr();
            r.frs(qq.fpath[k], r.u32());
        }
        if (r.bad) break;
    }
    if (r.bad || r.off != len) throw LspError(LSP_E_ARG, "malformed proof bytes");
    return p.release();
}

namespace {
// the flat, query-major arrays behind both views, built on first use and kept
// with the proof.  lsp_proof_view needs the first two matrices and the FRI openings
// (`error`: what keeps them from being flat arrays), the preprocessed view the third
struct Flat {
    std::vector<Fr> single;  // the roots on the wire, pow_witness
    struct Mat {
        std::vector<Fr> rows, paths;
        uint32_t path_len = 0;
        bool uniform = true;
    };
    std::vector<Mat> mats;
    std::vector<Fr> sibs, fpaths;
    std::vector<uint32_t> fri_path_lens;
    const char* error = nullptr;
};

// built once, under the proof's cache mutex (the caller holds it); never
// replaced afterwards, so pointers handed out stay valid until lsp_proof_free
const Flat& flat_of(const lsp_proof& p) {
    if (!p.view_cache) {
        auto f = std::make_shared<Flat>();
        const size_t nq = p.queries.size(), nr = p.roots.size(), nm = p.mats.size();
        for (const OpenedMat& m : p.mats)
            if (m.root_on_wire) f->single.push_back(m.root);
        f->single.push_back(p.pow_w);
        f->mats.resize(nm);
        for (size_t m = 0; m < nm && nq; ++m) f->mats[m].path_len = (uint32_t)p.queries[0].open[m].path.size();
        f->fri_path_lens.assign(nr, 0);
        for (size_t k = 0; k < nr && nq && p.queries[0].fpath.size() == nr; ++k)
            f->fri_path_lens[k] = (uint32_t)p.queries[0].fpath[k].size();
        for (auto& q : p.queries) {
            for (size_t m = 0; m < nm; ++m) {
                Flat::Mat& fm = f->mats[m];
                const auto& o = q.open[m];
                // the view holds one path length per tree (true of every proof
                // this library makes: all matrices of a tree have one height)
                if (o.row.size() != p.mats[m].width || o.path.size() != fm.path_len) fm.uniform = false;
                fm.rows.insert(fm.rows.end(), o.row.begin(), o.row.end());
                fm.paths.insert(fm.paths.end(), o.path.begin(), o.path.end());
            }
            if (f->error) continue;
            if (!f->mats[MAT_TRACE].uniform || !f->mats[MAT_QUOTIENT].uniform ||
                f->mats[MAT_QUOTIENT].path_len != f->mats[MAT_TRACE].path_len || q.sib.size() != nr ||
                q.fpath.size() != nr) {
                f->error = "proof queries are not uniform";
                continue;
            }
            for (size_t k = 0; k < nr && !f->error; ++k)
                if (q.fpath[k].size() != f->fri_path_lens[k]) f->error = "FRI paths differ in length";
            f->sibs.insert(f->sibs.end(), q.sib.begin(), q.sib.end());
            for (auto& fp : q.fpath) f->fpaths.insert(f->fpaths.end(), fp.begin(), fp.end());
        }
        p.view_cache = f;
    }
    return *std::static_pointer_cast<Flat>(p.view_cache);
}
const lsp_fr* as_lsp(const std::vector<Fr>& x) { return reinterpret_cast<const lsp_fr*>(x.data()); }
const lsp_fr* as_lsp(const Fr* x) { return reinterpret_cast<const lsp_fr*>(x); }
}  // namespace

void proof_prep_view(const lsp_proof& p, lsp_proof_preprocessed_view* v) {
    LSP_REQUIRE(p.mats.size() > MAT_PREP, LSP_E_STATE, "an LSPPRF02 proof has no preprocessed openings");
    std::lock_guard<std::mutex> g(p.cache_mu);
    const Flat::Mat& f = flat_of(p).mats[MAT_PREP];
    LSP_REQUIRE(f.uniform, LSP_E_STATE, "proof queries are not uniform");
    const OpenedMat& m = p.mats[MAT_PREP];
    std::memset(v, 0, sizeof *v);
    v->width = m.width;
    v->local = as_lsp(m.at(0));
    v->next = as_lsp(m.at(1));
    v->rows = as_lsp(f.rows);
    v->paths = as_lsp(f.paths);
    v->path_len = f.path_len;
}

void proof_view(const lsp_proof& p, lsp_proof_view* v) {
    std::lock_guard<std::mutex> g(p.cache_mu);
    const Flat& f = flat_of(p);
    if (f.error) throw LspError(LSP_E_STATE, f.error);
    const OpenedMat &t = p.mats[MAT_TRACE], &qm = p.mats[MAT_QUOTIENT];
    std::memset(v, 0, sizeof *v);
    v->degree_bits = p.log_h;
    v->log_quotient_chunks = p.log_q;
    v->width = t.width;
    v->num_queries = (uint32_t)p.queries.size();
    v->num_fri_rounds = (uint32_t)p.roots.size();
    v->final_poly_len = (uint32_t)p.final_poly.size();
    v->input_path_len = f.mats[MAT_TRACE].path_len;
    v->fri_path_lens = f.fri_path_lens.data();
    v->trace_commit = as_lsp(&f.single[MAT_TRACE]);
    v->quotient_commit = as_lsp(&f.single[MAT_QUOTIENT]);
    v->pow_witness = as_lsp(&f.single.back());
    v->trace_local = as_lsp(t.at(0));
    v->trace_next = as_lsp(t.at(1));
    v->quotient_chunks = as_lsp(qm.at(0));
    v->fri_commits = as_lsp(p.roots);
    v->final_poly = as_lsp(p.final_poly);
    v->trace_rows = as_lsp(f.mats[MAT_TRACE].rows);
    v->trace_paths = as_lsp(f.mats[MAT_TRACE].paths);
    v->quotient_rows = as_lsp(f.mats[MAT_QUOTIENT].rows);
    v->quotient_paths = as_lsp(f.mats[MAT_QUOTIENT].paths);
    v->fri_siblings = as_lsp(f.sibs);
    v->fri_paths = as_lsp(f.fpaths);
}

lsp_proof* proof_from_view(const lsp_proof_view& v) {
    // final_poly_len: a power of two (1 << log_final_poly_len) <= 2^20, the
    // lengths the wire format's reader accepts, so every view that builds a
    // handle serializes to bytes lsp_proof_deserialize reads back
    if (v.width == 0 || v.width > (1u << 20) || v.log_quotient_chunks > 20 || v.degree_bits > 40 ||
        v.num_fri_rounds > 64 || v.input_path_len > 64 || v.final_poly_len == 0 || v.final_poly_len > (1u << 20) ||
        (v.final_poly_len & (v.final_poly_len - 1)) != 0)
        throw LspError(LSP_E_ARG, "proof view out of range");
    const size_t w = v.width, q = (size_t)1 << v.log_quotient_chunks, nr = v.num_fri_rounds, pl = v.input_path_len;
    LSP_REQUIRE(v.trace_commit && v.quotient_commit && v.pow_witness && v.trace_local && v.trace_next &&
                    v.quotient_chunks && (nr == 0 || (v.fri_commits && v.fri_path_lens)) && v.final_poly,
                LSP_E_ARG, "null proof view field");
    LSP_REQUIRE(v.num_queries == 0 || (v.trace_rows && v.quotient_rows && v.fri_siblings &&
                                       (pl == 0 || (v.trace_paths && v.quotient_paths))),
                LSP_E_ARG, "null proof view query field");
    size_t fsum = 0;
    for (size_t k = 0; k < nr; ++k) {
        LSP_REQUIRE(v.fri_path_lens[k] <= 64, LSP_E_ARG, "FRI path too long");
        fsum += v.fri_path_lens[k];
    }
    LSP_REQUIRE(fsum == 0 || v.num_queries == 0 || v.fri_paths, LSP_E_ARG, "null FRI paths");
    auto rd = [](const lsp_fr* x, size_t n) {
        const Fr* f = reinterpret_cast<const Fr*>(x);
        for (size_t i = 0; i < n; ++i)
            LSP_REQUIRE(fr_words_lt_mod(f[i]), LSP_E_ARG, "proof element not reduced below the modulus");
        return std::vector<Fr>(f, f + n);
    };
    auto p = std::make_unique<lsp_proof>();
    p->log_h = v.degree_bits;
    p->log_q = v.log_quotient_chunks;
    p->mats = {OpenedMat(MAT_TRACE, v.width), OpenedMat(MAT_QUOTIENT, (uint32_t)q)};
    OpenedMat &t = p->mats[MAT_TRACE], &qm = p->mats[MAT_QUOTIENT];
    t.root = rd(v.trace_commit, 1)[0];
    qm.root = rd(v.quotient_commit, 1)[0];
    p->pow_w = rd(v.pow_witness, 1)[0];
    t.ys = rd(v.trace_local, w);
    const std::vector<Fr> tn = rd(v.trace_next, w);
    t.ys.insert(t.ys.end(), tn.begin(), tn.end());
    qm.ys = rd(v.quotient_chunks, q);
    p->roots = nr ? rd(v.fri_commits, nr) : std::vector<Fr>();
    p->final_poly = rd(v.final_poly, v.final_poly_len);
    p->queries.resize(v.num_queries);
    for (size_t i = 0; i < v.num_queries; ++i) {
        auto& qq = p->queries[i];
        qq.open.resize(2);
        qq.open[MAT_TRACE].row = rd(v.trace_rows + i * w, w);
        qq.open[MAT_TRACE].path = pl ? rd(v.trace_paths + i * pl, pl) : std::vector<Fr>();
        qq.open[MAT_QUOTIENT].row = rd(v.quotient_rows + i * q, q);
        qq.open[MAT_QUOTIENT].path = pl ? rd(v.quotient_paths + i * pl, pl) : std::vector<Fr>();
        qq.sib = nr ? rd(v.fri_siblings + i * nr, nr) : std::vector<Fr>();
        qq.fpath.resize(nr);
        size_t o = i * fsum;
        for (size_t k = 0; k < nr; ++k) {
            qq.fpath[k] = v.fri_path_lens[k] ? rd(v.fri_paths + o, v.fri_path_lens[k]) : std::vector<Fr>();
            o += v.fri_path_lens[k];
        }
    }
    return p.release();
}

}  // namespace lsp
