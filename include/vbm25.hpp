// vbm25.hpp -- C++ host mirror of the reference's interface for the query path, over the
// C ABI of vbm25.h (header only).
//
// The reference is Rust; there is no rustc in the build image, so the host side that a
// maintainer would write in Rust is mirrored here in C++ with the same
// names, argument meaning and error behaviour:
//   vbm25::intern        crates/bm25/src/vector.rs:19-35   (incl. the BLAKE3 keyed hash of long lexemes)
//   vbm25::Query         crates/bm25/src/vector.rs:96-134  (sorted unique 16-byte keys)
//   vbm25::Index::search crates/bm25/src/search.rs:28-36   (bm25::search, filter == true)
//   vbm25::search_growing, vbm25::merge_growing   crates/bm25/src/search.rs:83-135  (unsealed documents, host side)
//   vbm25::Segment::from_pages, vbm25::growing_from_pages   the relation's pages -> flat arrays (tape.rs, tuples.rs)
//   vbm25::DeviceGrowing::from_pages, vbm25::sealed_deleted_from_pages   the vectors tape read on the device; the sealed deleted flags
//   vbm25::DeviceVacuum::from_pages, ::maintain, DocFilter::remap(index, vacuum)   VACUUM's inputs read and consumed on the device
//   vbm25::Documents::bind, vbm25::DocTerms::evaluate   crates/bm25/src/evaluate.rs:22-74 for query batches with candidate rows, on the device
// Reference panics ("data corruption", "invalid data") and pgrx::error! become vbm25::Error.
#ifndef VBM25_HPP
#define VBM25_HPP

#include <algorithm>
#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "vbm25.h"

namespace vbm25 {

constexpr size_t WIDTH = 16;  // crates/bm25/src/lib.rs:37
using Key = std::array<uint8_t, WIDTH>;
using Hit = vbm25_hit;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};
inline void check(int rc) {
    if (rc != VBM25_OK) throw Error(rc, vbm25_last_error());
}

using Seed = std::array<uint8_t, 32>;  // MetaTuple.seed (tuples.rs:48-57)

// vector.rs:19-35: short lexemes are zero padded; lexemes of 16 bytes or more (or containing NUL) are the
// first 16 bytes of blake3::keyed_hash(seed, lexeme), last byte forced non-zero.
inline Key intern(const Seed &seed, std::string_view s) {
    Key k{};
    check(vbm25_intern(seed.data(), reinterpret_cast<const uint8_t *>(s.data()), s.size(), k.data()));
    return k;
}
// short path only (no index at hand): a lexeme that needs the hash raises VBM25_ERR_INVALID
inline Key intern(std::string_view s) {
    Key k{};
    check(vbm25_intern(nullptr, reinterpret_cast<const uint8_t *>(s.data()), s.size(), k.data()));
    return k;
}

// vector.rs:96-134
class Query {
  public:
    explicit Query(std::vector<Key> keys) : keys_(std::move(keys)) {
        for (size_t i = 1; i < keys_.size(); ++i)
            if (!(keys_[i - 1] < keys_[i])) throw Error(VBM25_ERR_INVALID, "invalid data");  // Query::new
    }
    // cast_tsvector_to_query, src/datatype/tsvector.rs:96-105: intern, sort, dedup
    template <class It>
    static Query from_tokens(It first, It last, const Seed *seed = nullptr) {
        std::vector<Key> keys;
        for (; first != last; ++first) keys.push_back(seed ? intern(*seed, *first) : intern(*first));
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        return Query(std::move(keys));
    }
    const std::vector<Key> &keys() const { return keys_; }
    size_t len() const { return keys_.size(); }
    bool is_empty() const { return keys_.empty(); }

  private:
    std::vector<Key> keys_;
};

// HBM-resident sealed segment.
class DocTerms;
class Index {
  public:
    Index(const vbm25_index_desc &desc, int device = 0) { check(vbm25_index_create(&desc, device, &h_)); }
    // of a segment in HBM (a compacted one: vbm25_index_maintain), on the segment's device; the segment is left as it was
    explicit Index(const vbm25_device_segment *segment) { check(vbm25_index_create_from_device(segment, &h_)); }
    ~Index() { vbm25_index_destroy(h_); }
    Index(const Index &) = delete;
    Index &operator=(const Index &) = delete;

    // bm25::search(&index, k, &query, |_| true): best first, at most k hits.
    std::vector<Hit> search(size_t k, const Query &query) const {
        std::vector<uint32_t> ids(query.len());
        if (!ids.empty())
            check(vbm25_lookup_terms(h_, query.keys()[0].data(), uint32_t(ids.size()), ids.data()));
        // unknown tokens are ignored (search.rs:59-61); key order == term id order
        ids.erase(std::remove(ids.begin(), ids.end(), UINT32_MAX), ids.end());
        const uint32_t off[2] = {0, uint32_t(ids.size())};
        std::vector<Hit> hits(k);
        uint32_t n = 0;
        check(vbm25_search_batch(h_, ids.data(), off, 1, uint32_t(k), hits.data(), &n));
        hits.resize(n);
        return hits;
    }
    // The batched form the GPU is built for: queries as CSR of ascending term ids.
    void search_batch(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, size_t k,
                      std::vector<Hit> &hits, std::vector<uint32_t> &n_hits) const {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        hits.resize(size_t(nq) * k);
        n_hits.resize(nq);
        check(vbm25_search_batch(h_, term_ids.data(), q_off.data(), nq, uint32_t(k), hits.data(), n_hits.data()));
    }
    // the forward index of the index's own sealed documents, made on the device from the index's arrays (vbm25_index_bind): document d
    // of the result is sealed document d.  Valid for this index only, which must outlive it; bind again after a compaction.
    inline DocTerms bind() const;
    vbm25_index *handle() const { return h_; }

  private:
    vbm25_index *h_ = nullptr;
};

// Lexemes back to back, as the resolver takes them: lexeme i = bytes[lex_off[i] .. lex_off[i + 1]), query q = lexemes
// q_lex[q] .. q_lex[q + 1].
struct LexemeBatch {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> lex_off{0};
    std::vector<uint32_t> q_lex{0};
    void add(std::string_view lexeme) {  // to the query that end_query() closes next
        bytes.insert(bytes.end(), lexeme.begin(), lexeme.end());
        lex_off.push_back(bytes.size());
    }
    void end_query() { q_lex.push_back(uint32_t(lex_off.size() - 1)); }
    uint32_t queries() const { return uint32_t(q_lex.size() - 1); }
    uint32_t lexemes() const { return uint32_t(lex_off.size() - 1); }
};

// The Query step on the device (vbm25_resolver): cast_tsvector_to_query + the key lookup of bm25::search for a batch -- lexemes or
// keys in, per query the ascending term ids out, the CSR every search entry point takes.  A ring of `depth` slots, first in first
// out; valid for its index only (on several GPUs a resolver on any replica serves all of them).
class Resolver {
  public:
    Resolver(const Index &index, const Seed *seed, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes, uint64_t max_bytes) {
        check(vbm25_resolver_create(index.handle(), seed ? seed->data() : nullptr, depth, max_queries, max_lexemes, max_bytes, &h_));
    }
    ~Resolver() { vbm25_resolver_destroy(h_); }
    Resolver(const Resolver &) = delete;
    Resolver &operator=(const Resolver &) = delete;

    void submit(const LexemeBatch &b) {
        check(vbm25_resolver_submit_lexemes(h_, b.bytes.data(), b.lex_off.data(), b.q_lex.data(), b.queries()));
        shape_.push_back({b.queries(), b.lexemes()});
    }
    void submit_keys(const std::vector<Key> &keys, const std::vector<uint32_t> &q_key) {
        check(vbm25_resolver_submit_keys(h_, keys.empty() ? nullptr : keys[0].data(), q_key.data(), uint32_t(q_key.size() - 1)));
        shape_.push_back({uint32_t(q_key.size() - 1), uint32_t(keys.size())});
    }
    // the oldest batch in flight (nothing in flight: the library's error)
    void collect(std::vector<uint32_t> &term_ids, std::vector<uint32_t> &q_off) {
        const std::array<uint32_t, 2> shape = shape_.empty() ? std::array<uint32_t, 2>{0, 0} : shape_.front();
        q_off.assign(size_t(shape[0]) + 1, 0);
        term_ids.assign(size_t(shape[1]) + 1, 0);
        uint32_t nq = 0;
        check(vbm25_resolver_collect(h_, term_ids.data(), q_off.data(), &nq));
        shape_.erase(shape_.begin());
        term_ids.resize(q_off[nq]);
    }
    int in_flight() const { return vbm25_resolver_in_flight(h_); }
    uint64_t device_bytes() const { return vbm25_resolver_device_bytes(h_); }
    vbm25_resolver *handle() const { return h_; }

  private:
    vbm25_resolver *h_ = nullptr;
    std::vector<std::array<uint32_t, 2>> shape_;  // per batch in flight: queries, lexemes
};

// bm25::search from the lexemes of tsvectors in one call (vbm25_search_batch_lexemes): hits is nq x k, n_hits nq
inline void search_batch_lexemes(const Index &index, const Seed *seed, const LexemeBatch &b, size_t k, std::vector<Hit> &hits,
                                 std::vector<uint32_t> &n_hits) {
    hits.resize(size_t(b.queries()) * k);
    n_hits.resize(b.queries());
    check(vbm25_search_batch_lexemes(index.handle(), seed ? seed->data() : nullptr, b.bytes.data(), b.lex_off.data(), b.q_lex.data(), b.queries(),
                                     uint32_t(k), hits.data(), n_hits.data()));
}

// intern for n lexemes at once on `device` (vbm25_intern_batch_device): byte for byte intern()'s keys
inline std::vector<Key> intern_batch(int device, const Seed *seed, const LexemeBatch &b) {
    std::vector<Key> keys(b.lexemes());
    check(vbm25_intern_batch_device(device, seed ? seed->data() : nullptr, b.bytes.data(), b.lex_off.data(), b.lexemes(),
                                    keys.empty() ? nullptr : keys[0].data()));
    return keys;
}

// tsvectors as the document cast takes them: LexemeBatch's packing plus the lexemes' position counts; a "query" of the batch is a
// document (add a lexeme with its count, end_document() closes the document).
struct DocumentBatch {
    LexemeBatch lexemes;
    std::vector<uint32_t> lex_count;
    std::vector<uint16_t> payload;  // 3 per document, or empty: documents nobody will index or append
    void add(std::string_view lexeme, uint32_t count) {
        lexemes.add(lexeme);
        lex_count.push_back(count);
    }
    void end_document() { lexemes.end_query(); }
    void end_document(const uint16_t (&ctid)[3]) {
        lexemes.end_query();
        payload.insert(payload.end(), ctid, ctid + 3);
    }
    uint32_t documents() const { return lexemes.queries(); }
};

struct GrowingDocs;
class DocTerms;
// The Document step on the device (RAII over vbm25_documents): cast_tsvector_to_document for a batch of tsvectors, the result kept in
// HBM.  DeviceSegment::from_documents makes the index of it, DeviceGrowing::append appends it, download() brings the CSR back.
class Documents {
  public:
    Documents(int device, const Seed *seed, const DocumentBatch &b) {
        check(vbm25_documents_cast(device, seed ? seed->data() : nullptr, b.lexemes.bytes.data(), b.lexemes.lex_off.data(), b.lex_count.data(),
                                   b.lexemes.q_lex.data(), b.documents(), b.payload.empty() ? nullptr : b.payload.data(), &h_));
    }
    // an owned handle of 0 documents, with or without payloads: what extend() grows
    static Documents empty(int device = 0, bool payload = false) {
        DocumentBatch b;
        if (payload) b.payload.assign(3, 0);  // (a non-NULL pointer: the handle is one with payloads)
        return Documents(device, nullptr, b);
    }
    Documents(Documents &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Documents(const Documents &) = delete;
    Documents &operator=(const Documents &) = delete;
    ~Documents() { vbm25_documents_free(h_); }  // (nothing for a handle a Caster handed out: it is the caster's)
    // vbm25_documents_extend: `src`'s documents behind this handle's, on the device.  This handle is an owned one.
    void extend(const Documents &src) { check(vbm25_documents_extend(h_, src.handle())); }
    uint32_t docs() const {
        uint32_t n = 0;
        check(vbm25_documents_info(h_, &n, nullptr, nullptr));
        return n;
    }
    uint64_t elements() const {
        uint64_t n = 0;
        check(vbm25_documents_info(h_, nullptr, &n, nullptr));
        return n;
    }
    uint64_t device_bytes() const { return vbm25_documents_device_bytes(h_); }
    // the CSR (payload empty when the cast had none) and, when asked for, the documents' lengths
    inline GrowingDocs download(std::vector<uint32_t> *doc_len = nullptr) const;
    // the documents' keys looked up in the vocabulary the resolver holds in HBM (vbm25_documents_bind): valid for its index only
    inline DocTerms bind(const Resolver &resolver) const;
    const vbm25_documents *handle() const { return h_; }

  private:
    friend class Caster;
    explicit Documents(const vbm25_documents *of_a_caster) : h_(const_cast<vbm25_documents *>(of_a_caster)) {}
    vbm25_documents *h_ = nullptr;
};

// The Document step as a ring (RAII over vbm25_caster): `depth` slots that keep their stream, events, pinned staging, device scratch
// and result arrays between casts.  submit() copies a batch in and enqueues it; collect() waits for the oldest batch and returns its
// Documents, which belongs to the slot: valid until the submit that takes the slot again (`depth` submits after its own) and no
// longer than the caster.  One thread drives a caster.  Move-only.
class Caster {
  public:
    Caster(int device, const Seed *seed, uint32_t depth, uint32_t max_docs, uint32_t max_lexemes, uint64_t max_bytes, uint32_t max_long_lexemes = 0) {
        check(vbm25_caster_create(device, seed ? seed->data() : nullptr, depth, max_docs, max_lexemes, max_bytes, max_long_lexemes, &h_));
    }
    Caster(Caster &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Caster(const Caster &) = delete;
    Caster &operator=(const Caster &) = delete;
    ~Caster() { vbm25_caster_free(h_); }
    void submit(const DocumentBatch &b) {
        check(vbm25_caster_submit(h_, b.lexemes.bytes.data(), b.lexemes.lex_off.data(), b.lex_count.data(), b.lexemes.q_lex.data(), b.documents(),
                                  b.payload.empty() ? nullptr : b.payload.data()));
    }
    Documents collect() {
        const vbm25_documents *d = nullptr;
        check(vbm25_caster_collect(h_, &d));
        return Documents(d);
    }
    int in_flight() const { return vbm25_caster_in_flight(h_); }
    uint64_t device_bytes() const { return vbm25_caster_device_bytes(h_); }
    // every allocation and creation the handle has made: it does not move after the constructor
    uint64_t allocations() const {
        uint64_t n = 0;
        check(vbm25_caster_info(h_, nullptr, nullptr, &n));
        return n;
    }
    vbm25_caster *handle() const { return h_; }

  private:
    vbm25_caster *h_ = nullptr;
};

// Cast documents bound to one index's vocabulary (RAII over vbm25_doc_terms): per document the ascending term ids of its known
// elements with their tfs, and its fieldnorm code, in HBM.  evaluate() is bm25::evaluate (evaluate.rs:22-74) for a batch of queries,
// each against its own candidate documents; the SQL operator `<&>` returns the negation of these values.  The index must outlive it.
// append() writes the bind of a delta behind the handle's documents (a live table's new rows; on a handle from Index::bind document
// base_docs() + g is growing document g); erase() marks documents dead, by index or by ctid, so that the rerank leaves them out;
// nobody else is inside a call on the handle meanwhile.
class Scorer;
class TidSet;
class DocTerms {
  public:
    DocTerms(const Documents &documents, const Resolver &resolver) { check(vbm25_documents_bind(documents.handle(), resolver.handle(), &h_)); }
    // the index's own sealed documents (vbm25_index_bind)
    explicit DocTerms(const Index &index) { check(vbm25_index_bind(index.handle(), &h_)); }
    DocTerms(DocTerms &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DocTerms(const DocTerms &) = delete;
    DocTerms &operator=(const DocTerms &) = delete;
    ~DocTerms() { vbm25_doc_terms_free(h_); }
    uint32_t docs() const {
        uint32_t n = 0;
        check(vbm25_doc_terms_info(h_, &n, nullptr, nullptr));
        return n;
    }
    uint64_t known() const {
        uint64_t n = 0;
        check(vbm25_doc_terms_info(h_, nullptr, &n, nullptr));
        return n;
    }
    uint64_t device_bytes() const { return vbm25_doc_terms_device_bytes(h_); }
    // the documents the handle was bound with (from Index::bind: the sealed ones)
    uint32_t base_docs() const { return vbm25_doc_terms_base_docs(h_); }
    // cast documents in HBM on the handle's device become documents docs() .. (vbm25_doc_terms_append_documents)
    void append(const Documents &delta, const Resolver &resolver) { check(vbm25_doc_terms_append_documents(h_, delta.handle(), resolver.handle())); }
    // the same from a host CSR; a document flagged deleted gets an empty run (vbm25_doc_terms_append)
    inline void append(const GrowingDocs &delta, const Resolver &resolver);
    // the documents docs[0 .. n) are dead (vbm25_doc_terms_delete): Scorer::topk and a Reranker leave them out, and a ctid names the
    // lowest live document that carries it; evaluate() and download() are unchanged.  Returns the documents that were live before.
    uint32_t erase(const uint32_t *docs, uint64_t n) {
        uint32_t n_new = 0;
        check(vbm25_doc_terms_delete(h_, docs, n, &n_new));
        return n_new;
    }
    // every document whose ctid is in the set is dead (vbm25_doc_terms_delete_tids).  payloads: the Documents whose payloads name the
    // documents the handle was bound with; none on a handle from Index::bind, whose ctids are the index's own.
    inline uint32_t erase(const TidSet &tids, const Documents *payloads = nullptr);
    uint32_t dead_docs() const { return vbm25_doc_terms_dead_docs(h_); }
    // the deletion bitmap, ceil(docs() / 64) words: document d at bit d & 63 of word d >> 6 (vbm25_doc_terms_read_dead)
    std::vector<uint64_t> read_dead() const {
        std::vector<uint64_t> w((size_t(docs()) + 63) / 64 + 1);
        check(vbm25_doc_terms_read_dead(h_, w.data()));
        w.pop_back();
        return w;
    }
    void download(std::vector<uint64_t> &start, std::vector<uint32_t> &term, std::vector<uint32_t> &tf) const {
        start.assign(size_t(docs()) + 1, 0);
        term.assign(known() + 1, 0);
        tf.assign(known() + 1, 0);
        check(vbm25_doc_terms_download(h_, start.data(), term.data(), tf.data()));
        term.pop_back();
        tf.pop_back();
    }
    // query q (term_ids[q_off[q] .. q_off[q+1]), ascending) scores the documents cand_doc[q_cand[q] .. q_cand[q+1]): aligned with cand_doc
    std::vector<double> evaluate(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, const std::vector<uint64_t> &q_cand,
                                 const std::vector<uint32_t> &cand_doc) const {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        if (q_cand.size() != q_off.size()) throw Error(VBM25_ERR_INVALID, "one candidate range per query");
        std::vector<double> scores(cand_doc.size() + 1);
        std::vector<uint32_t> ids(term_ids), docs(cand_doc);
        ids.push_back(0);  // (never NULL)
        docs.push_back(0);
        check(vbm25_evaluate_documents(h_, ids.data(), q_off.data(), nq, q_cand.data(), docs.data(), scores.data()));
        scores.pop_back();
        return scores;
    }
    // every query against every document: nq x docs(), row-major
    std::vector<double> evaluate(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off) const {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        std::vector<double> scores(size_t(nq) * docs() + 1);
        std::vector<uint32_t> ids(term_ids);
        ids.push_back(0);
        check(vbm25_evaluate_documents(h_, ids.data(), q_off.data(), nq, nullptr, nullptr, scores.data()));
        scores.pop_back();
        return scores;
    }
    // the rerank step on this handle, with everything kept between calls (vbm25_scorer_create); this object must outlive it
    inline Scorer scorer() const;
    const vbm25_doc_terms *handle() const { return h_; }

  private:
    vbm25_doc_terms *h_ = nullptr;
};
inline DocTerms Documents::bind(const Resolver &resolver) const { return DocTerms(*this, resolver); }
inline DocTerms Index::bind() const { return DocTerms(*this); }

// The rerank step on bound documents (RAII over vbm25_scorer): it keeps its stream, events, pinned staging and device buffers
// between calls.  evaluate() is DocTerms::evaluate through the handle; topk() returns each query's k best candidates -- score
// descending, then the position within the query's list ascending -- selected on the device.  One call at a time on a scorer (a
// mutex inside serialises them); several scorers on one DocTerms may run at once.  Move-only.
class Scorer {
  public:
    explicit Scorer(const DocTerms &documents) : t_(documents.handle()) { check(vbm25_scorer_create(documents.handle(), &h_)); }
    Scorer(Scorer &&o) noexcept : h_(o.h_), t_(o.t_) { o.h_ = nullptr; }
    Scorer(const Scorer &) = delete;
    Scorer &operator=(const Scorer &) = delete;
    ~Scorer() { vbm25_scorer_free(h_); }
    uint64_t device_bytes() const { return vbm25_scorer_device_bytes(h_); }
    std::vector<double> evaluate(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, const std::vector<uint64_t> &q_cand,
                                 const std::vector<uint32_t> &cand_doc) {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        if (q_cand.size() != q_off.size()) throw Error(VBM25_ERR_INVALID, "one candidate range per query");
        std::vector<double> scores(cand_doc.size() + 1);
        std::vector<uint32_t> ids(term_ids), docs(cand_doc);
        ids.push_back(0);  // (never NULL)
        docs.push_back(0);
        check(vbm25_scorer_evaluate(h_, ids.data(), q_off.data(), nq, q_cand.data(), docs.data(), scores.data()));
        scores.pop_back();
        return scores;
    }
    std::vector<double> evaluate(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off) {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        uint32_t docs = 0;  // (as of now: the handle may have grown)
        check(vbm25_doc_terms_info(t_, &docs, nullptr, nullptr));
        std::vector<double> scores(size_t(nq) * docs + 1);
        std::vector<uint32_t> ids(term_ids);
        ids.push_back(0);
        check(vbm25_scorer_evaluate(h_, ids.data(), q_off.data(), nq, nullptr, nullptr, scores.data()));
        scores.pop_back();
        return scores;
    }
    // ranks: nq x k, row-major, row q best first and zero behind n_ranks[q] = min(k, candidates of q)
    void topk(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, const std::vector<uint64_t> &q_cand,
              const std::vector<uint32_t> &cand_doc, uint32_t k, std::vector<vbm25_rank> &ranks, std::vector<uint32_t> &n_ranks) {
        if (q_cand.size() != q_off.size()) throw Error(VBM25_ERR_INVALID, "one candidate range per query");
        std::vector<uint32_t> docs(cand_doc);
        docs.push_back(0);
        topk_(term_ids, q_off, q_cand.data(), docs.data(), k, ranks, n_ranks);
    }
    // every document of the handle is a candidate of every query
    void topk(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, uint32_t k, std::vector<vbm25_rank> &ranks,
              std::vector<uint32_t> &n_ranks) {
        topk_(term_ids, q_off, nullptr, nullptr, k, ranks, n_ranks);
    }
    vbm25_scorer *handle() const { return h_; }

  private:
    void topk_(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, const uint64_t *q_cand, const uint32_t *cand_doc, uint32_t k,
               std::vector<vbm25_rank> &ranks, std::vector<uint32_t> &n_ranks) {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        std::vector<uint32_t> ids(term_ids);
        ids.push_back(0);
        ranks.assign(size_t(nq) * k + 1, vbm25_rank{0.0, 0, 0});
        n_ranks.assign(size_t(nq) + 1, 0);
        check(vbm25_scorer_topk(h_, ids.data(), q_off.data(), nq, q_cand, cand_doc, k, ranks.data(), n_ranks.data()));
        ranks.pop_back();
        n_ranks.pop_back();
    }
    vbm25_scorer *h_ = nullptr;
    const vbm25_doc_terms *t_ = nullptr;
};
inline Scorer DocTerms::scorer() const { return Scorer(*this); }

// The rerank step as a ring (RAII over vbm25_reranker): `depth` slots on a DocTerms, with the vocabulary and the seed of a resolver
// (both must outlive it).  submit() takes lexeme queries and candidates -- document indices, ctids (needs `payloads`, a Documents
// with payloads of the same documents, at construction; it may be freed afterwards) or none for the cross product -- and returns at
// once; collect() waits for the oldest batch and hands out Scorer::topk's rows, byte for byte what Resolver::submit / collect
// followed by Scorer::topk give.  Nothing is allocated after the constructor, except by a sync() that outgrows its room to spare.
// sync() brings the ctid directory up to the DocTerms' documents after DocTerms::append.  One thread drives a reranker.  Move-only.
// With the tag from_index, on a DocTerms made by Index::bind, the ctids are the index's own payloads (vbm25_reranker_create_from_index).
struct FromIndex {};
constexpr FromIndex from_index{};
class Reranker {
  public:
    Reranker(const DocTerms &documents, const Resolver &resolver, FromIndex, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes,
             uint64_t max_bytes, uint64_t max_candidates, uint32_t max_k) {
        check(vbm25_reranker_create_from_index(documents.handle(), resolver.handle(), depth, max_queries, max_lexemes, max_bytes, max_candidates,
                                               max_k, &h_));
    }
    Reranker(const DocTerms &documents, const Resolver &resolver, uint32_t depth, uint32_t max_queries, uint32_t max_lexemes, uint64_t max_bytes,
             uint64_t max_candidates, uint32_t max_k, const Documents *payloads = nullptr) {
        check(vbm25_reranker_create(documents.handle(), resolver.handle(), payloads ? payloads->handle() : nullptr, depth, max_queries, max_lexemes,
                                    max_bytes, max_candidates, max_k, &h_));
    }
    Reranker(Reranker &&o) noexcept : h_(o.h_), shape_(std::move(o.shape_)) { o.h_ = nullptr; }
    Reranker(const Reranker &) = delete;
    Reranker &operator=(const Reranker &) = delete;
    ~Reranker() { vbm25_reranker_free(h_); }
    // every document of the handle is a candidate of every query
    void submit(const LexemeBatch &b, uint32_t k) { submit_(b, nullptr, nullptr, nullptr, k); }
    // query q reranks the documents cand_doc[q_cand[q] .. q_cand[q+1])
    void submit(const LexemeBatch &b, uint32_t k, const std::vector<uint64_t> &q_cand, const std::vector<uint32_t> &cand_doc) {
        if (q_cand.size() != b.q_lex.size()) throw Error(VBM25_ERR_INVALID, "one candidate range per query");
        std::vector<uint32_t> docs(cand_doc);
        docs.push_back(0);  // (never NULL)
        submit_(b, q_cand.data(), docs.data(), nullptr, k);
    }
    // ... the documents that carry the ctids cand_tid[3 q_cand[q] .. 3 q_cand[q+1]) ([bi_hi, bi_lo, ip_posid] each)
    void submit_tids(const LexemeBatch &b, uint32_t k, const std::vector<uint64_t> &q_cand, const std::vector<uint16_t> &cand_tid) {
        if (q_cand.size() != b.q_lex.size()) throw Error(VBM25_ERR_INVALID, "one candidate range per query");
        if (cand_tid.size() % 3) throw Error(VBM25_ERR_INVALID, "three uint16_t per TID");
        std::vector<uint16_t> tids(cand_tid);
        tids.resize(tids.size() + 3, 0);
        submit_(b, q_cand.data(), nullptr, tids.data(), k);
    }
    // the queries as Scorer::topk's term ids (vbm25_reranker_submit_ids); q_cand empty: the cross product
    void submit_ids(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, uint32_t k, const std::vector<uint64_t> &q_cand = {},
                    const std::vector<uint32_t> &cand_doc = {}) {
        if (!q_cand.empty() && q_cand.size() != q_off.size()) throw Error(VBM25_ERR_INVALID, "one candidate range per query");
        std::vector<uint32_t> ids(term_ids), docs(cand_doc);
        ids.push_back(0);
        docs.push_back(0);
        const uint32_t nq = uint32_t(q_off.size() - 1);
        check(vbm25_reranker_submit_ids(h_, ids.data(), q_off.data(), nq, q_cand.empty() ? nullptr : q_cand.data(),
                                        q_cand.empty() ? nullptr : docs.data(), nullptr, k));
        shape_.push_back({nq, k});
    }
    // the oldest batch in flight (nothing in flight: the library's error): ranks is nq x k, row-major, row q best first and zero
    // behind n_ranks[q] = min(k, eligible entries of q); returns that batch's k
    uint32_t collect(std::vector<vbm25_rank> &ranks, std::vector<uint32_t> &n_ranks) {
        const std::array<uint32_t, 2> shape = shape_.empty() ? std::array<uint32_t, 2>{0, 1} : shape_.front();
        ranks.assign(size_t(shape[0]) * shape[1] + 1, vbm25_rank{0.0, 0, 0});
        n_ranks.assign(size_t(shape[0]) + 1, 0);
        uint32_t nq = 0, k = 0;
        check(vbm25_reranker_collect(h_, ranks.data(), n_ranks.data(), &nq, &k));
        shape_.erase(shape_.begin());
        ranks.pop_back();
        n_ranks.pop_back();
        return k;
    }
    int in_flight() const { return vbm25_reranker_in_flight(h_); }
    // the ctids of the documents appended since create or the last sync merged into the directory on the device (vbm25_reranker_sync)
    void sync() { check(vbm25_reranker_sync(h_)); }
    // the documents the directory covers
    uint32_t directory_docs() const { return vbm25_reranker_directory_docs(h_); }
    uint64_t device_bytes() const { return vbm25_reranker_device_bytes(h_); }
    // every allocation and creation the handle has made: it moves only in a sync() that grows
    uint64_t allocations() const {
        uint64_t n = 0;
        check(vbm25_reranker_info(h_, nullptr, nullptr, nullptr, &n));
        return n;
    }
    vbm25_reranker *handle() const { return h_; }

  private:
    void submit_(const LexemeBatch &b, const uint64_t *q_cand, const uint32_t *cand_doc, const uint16_t *cand_tid, uint32_t k) {
        check(vbm25_reranker_submit_lexemes(h_, b.bytes.data(), b.lex_off.data(), b.q_lex.data(), b.queries(), q_cand, cand_doc, cand_tid, k));
        shape_.push_back({b.queries(), k});  // (only a batch the library accepted is in the ring)
    }
    vbm25_reranker *h_ = nullptr;
    std::vector<std::array<uint32_t, 2>> shape_;  // per batch in flight: queries, k
};

class DeviceGrowing;
class DeviceVacuum;

// A set of ctids in the HBM of one device (RAII over vbm25_tid_set): VACUUM's dead TIDs, the TID bitmap of a heap scan.  tids: n x 3
// uint16_t ([bi_hi, bi_lo, ip_posid]) in any order, repeats allowed.  match() answers, for every document of an index or a growing
// segment, whether its payload is in the set, in the filters' packing; DocFilter::set_tids, DeviceGrowing::erase(const TidSet &) and
// DeviceVacuum::bulkdelete consume the set on the device.  Only ever read after it is made.
class TidSet {
  public:
    explicit TidSet(const std::vector<uint16_t> &tids, int device = 0) {
        if (tids.size() % 3) throw Error(VBM25_ERR_INVALID, "three uint16_t per TID");
        check(vbm25_tid_set_create(device, tids.empty() ? nullptr : tids.data(), tids.size() / 3, &h_));
    }
    ~TidSet() { vbm25_tid_set_free(h_); }
    TidSet(const TidSet &) = delete;
    TidSet &operator=(const TidSet &) = delete;
    TidSet(TidSet &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    uint64_t size() const {  // the distinct TIDs
        uint64_t n = 0;
        check(vbm25_tid_set_info(h_, &n, nullptr));
        return n;
    }
    int device() const {
        int d = 0;
        check(vbm25_tid_set_info(h_, nullptr, &d));
        return d;
    }
    // the distinct TIDs, size() x 3, ascending (vbm25_tid_set_read)
    std::vector<uint16_t> read() const {
        std::vector<uint16_t> t(3 * size());
        check(vbm25_tid_set_read(h_, t.empty() ? nullptr : t.data()));
        return t;
    }
    uint64_t device_bytes() const { return vbm25_tid_set_device_bytes(h_); }
    // words_per_bitmap(n_docs) words: bit d = sealed document d's payload is in the set; n_match, when given, the documents matched
    std::vector<uint64_t> match(const Index &index, uint32_t n_docs, uint32_t *n_match = nullptr) const {
        std::vector<uint64_t> w((size_t(n_docs) + 63) / 64 + 1);
        check(vbm25_tid_set_match_index(h_, index.handle(), w.data(), n_match));
        w.pop_back();
        return w;
    }
    // the same over a growing segment's documents, deleted ones included (vbm25_tid_set_match_growing)
    inline std::vector<uint64_t> match(const DeviceGrowing &growing, uint32_t *n_match = nullptr) const;
    const vbm25_tid_set *handle() const { return h_; }

  private:
    vbm25_tid_set *h_ = nullptr;
};
inline uint32_t DocTerms::erase(const TidSet &tids, const Documents *payloads) {
    uint32_t n_new = 0;
    check(vbm25_doc_terms_delete_tids(h_, tids.handle(), payloads ? payloads->handle() : nullptr, &n_new));
    return n_new;
}

// F document bitmaps of one index in HBM (vbm25_filter): bit d % 64 of word d / 64 of bitmap i set = document d may be returned.
// Optionally F growing bitmaps for one uploaded growing segment (set_growing): bit g = growing document g may be returned.
class DocFilter {
  public:
    static size_t words_per_bitmap(uint32_t n_docs) { return (size_t(n_docs) + 63) / 64; }
    // words: n_bitmaps x words_per_bitmap(n_docs), or empty for all bits zero
    DocFilter(Index &index, uint32_t n_bitmaps, const std::vector<uint64_t> &words = {}) {
        check(vbm25_filter_create(index.handle(), n_bitmaps, words.empty() ? nullptr : words.data(), &h_));
    }
    ~DocFilter() { vbm25_filter_destroy(h_); }
    DocFilter(const DocFilter &) = delete;
    DocFilter &operator=(const DocFilter &) = delete;
    DocFilter(DocFilter &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    // This filter carried across vbm25_index_maintain on the device (vbm25_filter_remap): sealed_deleted (empty: none; else
    // words_per_bitmap(old n_docs) words, DELETED polarity) and the n_grow growing documents' deleted flags (empty: none deleted) are
    // what the compaction got; new_index is the index of the compacted segment (an Index, or a replica of a MultiIndex).  The new
    // filter has no growing bitmaps; this one is only read and stays valid.
    DocFilter remap(vbm25_index *new_index, const std::vector<uint64_t> &sealed_deleted = {}, uint32_t n_grow = 0,
                    const std::vector<uint8_t> &growing_deleted = {}) const {
        if (!growing_deleted.empty() && growing_deleted.size() != n_grow) throw Error(VBM25_ERR_INVALID, "one deleted flag per growing document");
        vbm25_filter *h = nullptr;
        check(vbm25_filter_remap(h_, sealed_deleted.empty() ? nullptr : sealed_deleted.data(), n_grow,
                                 growing_deleted.empty() ? nullptr : growing_deleted.data(), new_index, &h));
        return DocFilter(h);
    }
    DocFilter remap(const Index &new_index, const std::vector<uint64_t> &sealed_deleted = {}, uint32_t n_grow = 0,
                    const std::vector<uint8_t> &growing_deleted = {}) const {
        return remap(new_index.handle(), sealed_deleted, n_grow, growing_deleted);
    }
    // ... with the three deletion arguments taken from the handle the compaction read (vbm25_filter_remap_device)
    inline DocFilter remap(vbm25_index *new_index, const DeviceVacuum &in) const;
    inline DocFilter remap(const Index &new_index, const DeviceVacuum &in) const;
    // bitmap i back on the host (vbm25_filter_read): n_words = words_per_bitmap(n_docs), or of the growing documents covered
    std::vector<uint64_t> read(uint32_t i, size_t n_words, bool growing = false) const {
        std::vector<uint64_t> w(n_words ? n_words : 1);
        check(vbm25_filter_read(h_, i, growing ? 1 : 0, w.data()));
        w.resize(n_words);
        return w;
    }
    void update(uint32_t i, const std::vector<uint64_t> &words) { check(vbm25_filter_update(h_, i, words.data())); }
    void *device_words(uint32_t i) {
        void *p = nullptr;
        check(vbm25_filter_device_words(h_, i, &p));
        return p;
    }
    // growing bitmaps: n_bitmaps x words_per_bitmap(n_grow), or empty for all bits zero; a NULL segment removes them
    inline void set_growing(const DeviceGrowing *growing, const std::vector<uint64_t> &words = {});
    void update_growing(uint32_t i, const std::vector<uint64_t> &words) { check(vbm25_filter_update_growing(h_, i, words.data())); }
    // after DeviceGrowing::append: the growing bitmaps extended in place to the segment's document count.  words: n_bitmaps x
    // words_per_bitmap(d) for the d new documents (bit j: growing document old count + j), or empty for all bits zero.  The
    // addresses growing_device_words returns may change.
    inline void extend_growing(const DeviceGrowing &growing, const std::vector<uint64_t> &words = {});
    // sealed bitmap i = "the document's payload is in the set" (invert: "is not"), made on the device; with `growing` (the segment of
    // this filter's growing bitmaps, at its current document count) growing bitmap i likewise (vbm25_filter_set_tids)
    inline void set_tids(uint32_t i, const TidSet &tids, bool invert = false, const DeviceGrowing *growing = nullptr);
    void *growing_device_words(uint32_t i) {
        void *p = nullptr;
        check(vbm25_filter_growing_device_words(h_, i, &p));
        return p;
    }
    // the exact filtered top-k: query q returns documents of bitmap q_filter[q] only (UINT32_MAX: every document)
    void search_batch(const Index &index, const std::vector<uint32_t> &q_filter, const std::vector<uint32_t> &term_ids,
                      const std::vector<uint32_t> &q_off, size_t k, std::vector<Hit> &hits, std::vector<uint32_t> &n_hits) const {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        if (q_filter.size() != nq) throw Error(VBM25_ERR_INVALID, "one selector per query");
        hits.resize(size_t(nq) * k);
        n_hits.resize(nq);
        check(vbm25_search_batch_filtered(index.handle(), h_, q_filter.data(), term_ids.data(), q_off.data(), nq, uint32_t(k),
                                          hits.data(), n_hits.data()));
    }
    vbm25_filter *handle() const { return h_; }

  private:
    explicit DocFilter(vbm25_filter *h) : h_(h) {}
    vbm25_filter *h_ = nullptr;
};

// The sealed segment replicated on several GPUs of one node (vbm25_multi): uploaded from the host once, or made of a device segment
// (a compacted one) on the segment's device, which devices[0] must name; the other replicas are copied GPU to GPU.
class MultiIndex {
  public:
    MultiIndex(const vbm25_index_desc &desc, const std::vector<int> &devices) {
        check(vbm25_multi_create(&desc, devices.data(), int(devices.size()), &h_));
    }
    MultiIndex(const vbm25_device_segment *segment, const std::vector<int> &devices) {
        check(vbm25_multi_create_from_device(segment, devices.data(), int(devices.size()), &h_));
    }
    ~MultiIndex() { vbm25_multi_destroy(h_); }
    MultiIndex(const MultiIndex &) = delete;
    MultiIndex &operator=(const MultiIndex &) = delete;
    int device_count() const { return vbm25_multi_device_count(h_); }
    // replica i (borrowed): what that replica's DocFilter::remap, filters and growing segments are made on
    vbm25_index *replica(int i) const {
        vbm25_index *ix = nullptr;
        check(vbm25_multi_index(h_, i, &ix));
        return ix;
    }
    void search_batch(const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, size_t k, std::vector<Hit> &hits,
                      std::vector<uint32_t> &n_hits) const {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        hits.resize(size_t(nq) * k);
        n_hits.resize(nq);
        check(vbm25_multi_search_batch(h_, term_ids.data(), q_off.data(), nq, uint32_t(k), hits.data(), n_hits.data()));
    }
    vbm25_multi *handle() const { return h_; }

  private:
    vbm25_multi *h_ = nullptr;
};

// Host copy of a flattened sealed segment (RAII over vbm25_segment).
class Segment {
  public:
    // A bm25 index relation in the reference's on-disk format (PostgreSQL 8 KiB pages): Meta -> Jump ->
    // documents / tokens / summaries / blocks tapes (the walk of maintain.rs:104-161).
    static Segment from_pages(vbm25_read_page_fn read_page, void *ctx) {
        vbm25_segment *h = nullptr;
        check(vbm25_segment_from_pages(read_page, ctx, &h));
        return Segment(h);
    }
    explicit Segment(vbm25_segment *h) : h_(h) {}
    Segment(Segment &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Segment(const Segment &) = delete;
    Segment &operator=(const Segment &) = delete;
    ~Segment() { vbm25_segment_free(h_); }
    vbm25_index_desc desc() const {
        vbm25_index_desc d;
        check(vbm25_segment_desc(h_, &d));
        return d;
    }

  private:
    vbm25_segment *h_;
};

// A sealed segment in HBM (RAII over vbm25_device_segment): Index(seg.handle()) and MultiIndex(seg.handle(), devices) make
// indexes of it, download() the host copy.
class DeviceSegment {
  public:
    // The device reader: the relation's sealed segment read into the HBM of `device` without a host copy of the index (the host
    // follows the page chains, kernels parse, validate and flatten).  Accepts and refuses what Segment::from_pages does.
    static DeviceSegment from_pages(vbm25_read_page_fn read_page, void *ctx, int device = 0) {
        vbm25_device_segment *h = nullptr;
        check(vbm25_device_segment_from_pages(read_page, ctx, device, &h));
        return DeviceSegment(h);
    }
    // The index ambuild makes of cast documents (vbm25_device_segment_build_documents): document i = doc id i, the vocabulary = their
    // distinct keys; sorted, ranked and encoded on the documents' device.
    static DeviceSegment from_documents(const Documents &documents, double k1, double b) {
        vbm25_device_segment *h = nullptr;
        check(vbm25_device_segment_build_documents(documents.handle(), k1, b, &h));
        return DeviceSegment(h);
    }
    explicit DeviceSegment(vbm25_device_segment *h) : h_(h) {}
    DeviceSegment(DeviceSegment &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DeviceSegment(const DeviceSegment &) = delete;
    DeviceSegment &operator=(const DeviceSegment &) = delete;
    ~DeviceSegment() { vbm25_device_segment_free(h_); }
    Segment download() const {
        vbm25_segment *s = nullptr;
        check(vbm25_device_segment_download(h_, &s));
        return Segment(s);
    }
    // The device writer (the inverse of from_pages): the pages a flush of the segment allocates; the flush with the i-th allocation
    // getting page_ids[i] (empty: first_page + i), one write_page call per finished image; a whole fresh relation (build.rs:22-71).
    uint32_t page_count() const {
        uint32_t n = 0;
        check(vbm25_device_segment_page_count(h_, &n));
        return n;
    }
    vbm25_flushed write_pages(vbm25_write_page_fn write_page, void *ctx, const std::vector<uint32_t> &page_ids = {}, uint32_t first_page = 0) const {
        vbm25_flushed f;
        check(vbm25_device_segment_write_pages(h_, page_ids.empty() ? nullptr : page_ids.data(), (uint32_t)page_ids.size(), first_page, write_page,
                                               ctx, &f));
        return f;
    }
    uint32_t write_relation(vbm25_write_page_fn write_page, void *ctx, const uint8_t *seed32 = nullptr) const {
        uint32_t n = 0;
        check(vbm25_device_segment_write_relation(h_, seed32, write_page, ctx, &n));
        return n;
    }
    const vbm25_device_segment *handle() const { return h_; }

  private:
    vbm25_device_segment *h_;
};

// The growing (unsealed) segment, search.rs:83-135: documents as CSR over their VectorTuple elements.
struct GrowingDocs {
    std::vector<uint64_t> start{0};      // n + 1 offsets into key / tf
    std::vector<Key> key;                // Element.key
    std::vector<uint32_t> tf;            // Element.value
    std::vector<uint8_t> fieldnorm;      // VectorTuple::_2.fieldnorm
    std::vector<uint16_t> payload;       // VectorTuple::_0.payload, n x 3
    std::vector<uint8_t> deleted;        // VectorTuple::_0.deleted
    size_t size() const { return start.size() - 1; }
};
// The unsealed documents of a relation (vectors tape from Jump.ptr_vectors; VectorTuple _2 / _1 / _0).
inline GrowingDocs growing_docs_of(vbm25_growing *g);  // (takes the handle over)
inline GrowingDocs growing_from_pages(vbm25_read_page_fn read_page, void *ctx) {
    vbm25_growing *g = nullptr;
    check(vbm25_growing_from_pages(read_page, ctx, &g));
    return growing_docs_of(g);
}
inline GrowingDocs growing_docs_of(vbm25_growing *g) {
    vbm25_growing_desc d;
    const int rc = vbm25_growing_get_desc(g, &d);
    GrowingDocs out;
    if (rc == VBM25_OK) {
        out.start.assign(d.start, d.start + d.n_docs + 1);
        out.key.resize(d.n_elements);
        if (d.n_elements) std::memcpy(out.key[0].data(), d.key, 16 * d.n_elements);
        out.tf.assign(d.tf, d.tf + d.n_elements);
        out.fieldnorm.assign(d.fieldnorm, d.fieldnorm + d.n_docs);
        if (d.payload) out.payload.assign(d.payload, d.payload + 3ull * d.n_docs);  // (NULL: documents cast without payloads)
        out.deleted.assign(d.deleted, d.deleted + d.n_docs);
    }
    vbm25_growing_free(g);
    check(rc);
    return out;
}
using GrowingDesc = GrowingDocs;
inline void DocTerms::append(const GrowingDocs &delta, const Resolver &resolver) {
    vbm25_growing_desc d{};
    d.n_docs = uint32_t(delta.size());
    d.n_elements = delta.tf.size();
    d.start = delta.start.data();
    d.key = delta.key.empty() ? nullptr : delta.key[0].data();
    d.tf = delta.tf.data();
    d.fieldnorm = delta.fieldnorm.data();
    d.payload = delta.payload.empty() ? nullptr : delta.payload.data();  // (none: a delta without payloads)
    d.deleted = delta.deleted.empty() ? nullptr : delta.deleted.data();
    check(vbm25_doc_terms_append(h_, &d, resolver.handle()));
}
inline GrowingDocs Documents::download(std::vector<uint32_t> *doc_len) const {
    vbm25_growing *g = nullptr;
    if (doc_len) doc_len->assign(docs(), 0);
    check(vbm25_documents_download(h_, &g, doc_len && !doc_len->empty() ? doc_len->data() : nullptr));
    return growing_docs_of(g);
}
// DocumentTuple.deleted of every sealed document of a relation as the DELETED words vbm25_index_maintain and vbm25_filter_remap
// take (bit d % 64 of word d / 64); n_docs, when given, receives the document count (vbm25_sealed_deleted_from_pages)
inline std::vector<uint64_t> sealed_deleted_from_pages(vbm25_read_page_fn read_page, void *ctx, uint32_t *n_docs = nullptr) {
    uint32_t n = 0;
    check(vbm25_sealed_deleted_from_pages(read_page, ctx, nullptr, 0, &n, nullptr));
    std::vector<uint64_t> words((size_t(n) + 63) / 64);
    check(vbm25_sealed_deleted_from_pages(read_page, ctx, words.data(), uint32_t(words.size()), &n, nullptr));
    if (n_docs) *n_docs = n;
    return words;
}
// Scores the unsealed documents with the sealed segment's statistics (host code, as in the reference).
inline std::vector<Hit> search_growing(const vbm25_index_desc &desc, const Query &query, size_t k,
                                       const GrowingDocs &g) {
    std::vector<Hit> hits(k);
    uint32_t n = 0;
    check(vbm25_growing_search(&desc, query.is_empty() ? nullptr : query.keys()[0].data(), uint32_t(query.len()),
                               uint32_t(k), uint32_t(g.size()), g.start.data(),
                               g.key.empty() ? nullptr : g.key[0].data(), g.tf.data(), g.fieldnorm.data(),
                               g.payload.data(), g.deleted.empty() ? nullptr : g.deleted.data(), hits.data(), &n));
    hits.resize(n);
    return hits;
}
// search.rs:83-135 + 301-313: top-k of the union of the sealed hits (device) and the growing hits
// (host), best first; on equal scores sealed hits come first.
inline std::vector<Hit> merge_growing(const std::vector<Hit> &sealed, const std::vector<Hit> &grow, size_t k) {
    std::vector<Hit> out(k);
    uint32_t n = 0;
    check(vbm25_merge_hits(sealed.data(), uint32_t(sealed.size()), grow.data(), uint32_t(grow.size()), uint32_t(k),
                           out.data(), &n));
    out.resize(n);
    return out;
}

// The growing segment of one index in HBM (vbm25_device_growing): the device form of search_growing + merge_growing for a whole
// batch.  append() the documents the relation gained and erase() those it marked deleted; both change the segment in place.
class DeviceGrowing {
  public:
    DeviceGrowing(Index &index, const GrowingDocs &g) {
        const vbm25_growing_desc d = desc_of(g);
        check(vbm25_growing_upload(index.handle(), &d, &h_));
    }
    // The growing segment of a relation read on the index's device (vbm25_device_growing_from_pages: the host follows the vectors
    // tape's page chain, kernels parse, validate and flatten): the segment DeviceGrowing(index, growing_from_pages(...)) makes.
    // `csr`, when given, receives the CSR copied back from the device (growing_from_pages' arrays).
    static DeviceGrowing from_pages(Index &index, vbm25_read_page_fn read_page, void *ctx, GrowingDocs *csr = nullptr) {
        DeviceGrowing out;
        vbm25_growing *g = nullptr;
        check(vbm25_device_growing_from_pages(index.handle(), read_page, ctx, &out.h_, csr ? &g : nullptr));
        if (csr) *csr = growing_docs_of(g);
        return out;
    }
    DeviceGrowing(DeviceGrowing &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    // the new documents only: document i of `delta` becomes growing document docs() + i (vbm25_device_growing_append)
    void append(const GrowingDocs &delta) {
        const vbm25_growing_desc d = desc_of(delta);
        check(vbm25_device_growing_append(h_, &d));
    }
    // the same from cast documents in HBM on the segment's device (vbm25_device_growing_append_documents)
    void append(const Documents &delta) { check(vbm25_device_growing_append_documents(h_, delta.handle())); }
    // growing indices below docs(), any order (vbm25_device_growing_delete)
    void erase(const std::vector<uint32_t> &g) { check(vbm25_device_growing_delete(h_, g.data(), uint32_t(g.size()))); }
    // every growing document whose payload is in the set, found on the device (vbm25_device_growing_delete_tids); returns the
    // documents matched, those already deleted included
    uint32_t erase(const TidSet &tids) {
        uint32_t n = 0;
        check(vbm25_device_growing_delete_tids(h_, tids.handle(), &n));
        return n;
    }
    uint32_t docs() const { return vbm25_device_growing_docs(h_); }
    ~DeviceGrowing() { vbm25_device_growing_free(h_); }
    DeviceGrowing(const DeviceGrowing &) = delete;
    DeviceGrowing &operator=(const DeviceGrowing &) = delete;
    uint64_t device_bytes() const { return vbm25_device_growing_bytes(h_); }
    // per query: the sealed top-k and the growing documents' merged (sealed first on equal scores)
    void search_batch(const Index &index, const std::vector<uint32_t> &term_ids, const std::vector<uint32_t> &q_off, size_t k,
                      std::vector<Hit> &hits, std::vector<uint32_t> &n_hits) const {
        const uint32_t nq = uint32_t(q_off.size() - 1);
        hits.resize(size_t(nq) * k);
        n_hits.resize(nq);
        check(vbm25_search_batch_growing(index.handle(), h_, term_ids.data(), q_off.data(), nq, uint32_t(k), hits.data(),
                                         n_hits.data()));
    }
    vbm25_device_growing *handle() const { return h_; }

  private:
    DeviceGrowing() = default;
    static vbm25_growing_desc desc_of(const GrowingDocs &g) {
        vbm25_growing_desc d{};
        d.n_docs = uint32_t(g.size());
        d.n_elements = g.tf.size();
        d.start = g.start.data();
        d.key = g.key.empty() ? nullptr : g.key[0].data();
        d.tf = g.tf.data();
        d.fieldnorm = g.fieldnorm.data();
        d.payload = g.payload.data();
        d.deleted = g.deleted.empty() ? nullptr : g.deleted.data();
        return d;
    }
    vbm25_device_growing *h_ = nullptr;
};

// A relation's compaction inputs in HBM on the index's device (RAII over vbm25_device_vacuum): the sealed documents' deleted words and
// the growing segment's CSR, read from the pages by kernels.  maintain() is vbm25_index_maintain_device: VACUUM's compaction with
// these inputs read in place; DocFilter::remap(new_index, vacuum) carries the filters across.  The handle is only read, except by
// bulkdelete(), which must not run beside a maintain() or a remap() of the same handle.
class DeviceVacuum {
  public:
    static DeviceVacuum from_pages(Index &index, vbm25_read_page_fn read_page, void *ctx) {
        DeviceVacuum out;
        check(vbm25_device_vacuum_from_pages(index.handle(), read_page, ctx, &out.h_));
        check(vbm25_device_vacuum_info(out.h_, &out.n_sealed, &out.n_sealed_deleted, &out.n_grow, &out.n_grow_deleted, &out.n_elements));
        return out;
    }
    DeviceVacuum(DeviceVacuum &&o) noexcept
        : n_sealed(o.n_sealed), n_sealed_deleted(o.n_sealed_deleted), n_grow(o.n_grow), n_grow_deleted(o.n_grow_deleted),
          n_elements(o.n_elements), h_(o.h_) {
        o.h_ = nullptr;
    }
    DeviceVacuum(const DeviceVacuum &) = delete;
    DeviceVacuum &operator=(const DeviceVacuum &) = delete;
    ~DeviceVacuum() { vbm25_device_vacuum_free(h_); }
    // the compacted segment; relabel, when given, receives n_sealed + n_grow entries: old id -> new id or UINT32_MAX
    DeviceSegment maintain(const Index &index, std::vector<uint32_t> *relabel = nullptr) const {
        if (relabel) relabel->assign(size_t(n_sealed) + n_grow, 0);
        vbm25_device_segment *seg = nullptr;
        check(vbm25_index_maintain_device(index.handle(), h_, relabel ? relabel->data() : nullptr, &seg));
        return DeviceSegment(seg);
    }
    // the two deletion inputs back on the host (vbm25_device_vacuum_read)
    void read(std::vector<uint64_t> &sealed_deleted_words, std::vector<uint8_t> &growing_deleted) const {
        sealed_deleted_words.assign((size_t(n_sealed) + 63) / 64, 0);
        growing_deleted.assign(n_grow, 0);
        check(vbm25_device_vacuum_read(h_, sealed_deleted_words.data(), growing_deleted.data()));
    }
    // bulkdelete.rs on the handle (vbm25_device_vacuum_bulkdelete): every sealed document of `index` (the one the handle was read
    // for) and every growing document whose payload is in the set is flagged deleted.  Returns {sealed, growing}: the documents that
    // were live before and are deleted now; the counts of this object follow.
    std::pair<uint32_t, uint32_t> bulkdelete(const Index &index, const TidSet &tids) {
        uint32_t ns = 0, ng = 0;
        check(vbm25_device_vacuum_bulkdelete(h_, index.handle(), tids.handle(), &ns, &ng));
        check(vbm25_device_vacuum_info(h_, nullptr, &n_sealed_deleted, nullptr, &n_grow_deleted, nullptr));
        return {ns, ng};
    }
    const vbm25_device_vacuum *handle() const { return h_; }
    uint32_t n_sealed = 0, n_sealed_deleted = 0, n_grow = 0, n_grow_deleted = 0;
    uint64_t n_elements = 0;

  private:
    DeviceVacuum() = default;
    vbm25_device_vacuum *h_ = nullptr;
};

inline DocFilter DocFilter::remap(vbm25_index *new_index, const DeviceVacuum &in) const {
    vbm25_filter *h = nullptr;
    check(vbm25_filter_remap_device(h_, in.handle(), new_index, &h));
    return DocFilter(h);
}
inline DocFilter DocFilter::remap(const Index &new_index, const DeviceVacuum &in) const { return remap(new_index.handle(), in); }

inline void DocFilter::set_growing(const DeviceGrowing *growing, const std::vector<uint64_t> &words) {
    check(vbm25_filter_set_growing(h_, growing ? growing->handle() : nullptr, words.empty() ? nullptr : words.data()));
}

inline void DocFilter::extend_growing(const DeviceGrowing &growing, const std::vector<uint64_t> &words) {
    check(vbm25_filter_extend_growing(h_, growing.handle(), words.empty() ? nullptr : words.data()));
}

inline void DocFilter::set_tids(uint32_t i, const TidSet &tids, bool invert, const DeviceGrowing *growing) {
    check(vbm25_filter_set_tids(h_, i, tids.handle(), invert ? 1 : 0, growing ? growing->handle() : nullptr));
}

inline std::vector<uint64_t> TidSet::match(const DeviceGrowing &growing, uint32_t *n_match) const {
    std::vector<uint64_t> w((size_t(growing.docs()) + 63) / 64 + 1);
    check(vbm25_tid_set_match_growing(h_, growing.handle(), w.data(), n_match));
    w.pop_back();
    return w;
}

// per query: the sealed and the growing records merged, query q taking bitmap q_filter[q] of `filter` on both segments
// (UINT32_MAX: every document); the filter's growing bitmaps must be those of `growing`
inline void search_batch_growing_filtered(const Index &index, const DeviceGrowing &growing, const DocFilter &filter,
                                          const std::vector<uint32_t> &q_filter, const std::vector<uint32_t> &term_ids,
                                          const std::vector<uint32_t> &q_off, size_t k, std::vector<Hit> &hits,
                                          std::vector<uint32_t> &n_hits) {
    const uint32_t nq = uint32_t(q_off.size() - 1);
    if (q_filter.size() != nq) throw Error(VBM25_ERR_INVALID, "one selector per query");
    hits.resize(size_t(nq) * k);
    n_hits.resize(nq);
    check(vbm25_search_batch_growing_filtered(index.handle(), growing.handle(), filter.handle(), q_filter.data(), term_ids.data(),
                                              q_off.data(), nq, uint32_t(k), hits.data(), n_hits.data()));
}

}  // namespace vbm25
#endif
