// device_segment.h -- a sealed segment whose arrays live in HBM (vbm25_device_segment): what csrc/flush.hip builds and
// csrc/index.hip (vbm25_index_create_from_device) makes an index of without a round trip through the host.
// Shared by the two HIP translation units of libvbm25; not part of the ABI.
#ifndef VBM25_DEVICE_SEGMENT_H
#define VBM25_DEVICE_SEGMENT_H

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/vbm25.h"
#include "hip_host.h"

// The values flush.rs:40-158 writes to the Token / Summary / Block / Document tapes (the arrays of vbm25_index_desc), in the
// HBM of `device`; the few things the host needs again (keys for the token lookup, block counts) as host copies.
struct vbm25_device_segment {
    int device = 0;
    double k1 = 1.2, b = 0.75;
    uint32_t n_docs = 0, n_terms = 0, n_blocks = 0;
    uint64_t sum_len = 0, blob_bytes = 0;
    std::vector<uint8_t> term_key;           // n_terms x 16, ascending
    std::vector<uint32_t> term_first_block;  // n_terms + 1
    std::vector<uint32_t> term_df;           // n_terms
    std::vector<uint64_t> term_bytes;        // per term: the algorithmic bytes of its postings (vbm25_query_bytes without the 14 k)
    std::vector<uint32_t> token_term;        // synthetic corpora only: token number -> term id
    vbm25::HbmArray d_term_df, d_term_wand_fn, d_term_wand_tf, d_term_first_block, d_blk_min, d_blk_max, d_blk_n, d_blk_wand_fn,
        d_blk_wand_tf, d_blk_meta_doc, d_blk_meta_tf, d_blk_off8, d_blob, d_doc_fieldnorm, d_doc_payload;
};

// A relation's compaction inputs in HBM (vbm25_device_vacuum_from_pages, csrc/pages_device.hip): the sealed documents' deleted flags
// as ceil(n_sealed / 64) words in DELETED polarity and the growing segment's CSR (vbm25_growing_desc's arrays, start[0] == 0, keys
// strictly ascending inside a document).  Only ever read after it is made: vbm25_index_maintain_device and
// vbm25_filter_remap_device take the planes in place.
struct vbm25_device_vacuum {
    int device = 0;
    uint32_t n_sealed = 0, n_sealed_deleted = 0, n_grow = 0, n_grow_deleted = 0;
    uint64_t n_elements = 0;
    vbm25::HbmArray d_sealed_deleted, d_start, d_key, d_tf, d_fieldnorm, d_deleted, d_payload;
};

// Cast documents in HBM (vbm25_documents_cast, csrc/cast.hip): the CSR cast_tsvector_to_document makes of a batch of tsvectors -- start
// (n_docs + 1, start[0] == 0), per element the key and the tf (keys strictly ascending inside a document), per document the length, its
// fieldnorm code and, when the caller gave them, the payload.  Only ever read after it is made, except by vbm25_documents_extend, which
// appends to an owned handle.  The arrays may be larger than the documents need (a caster's slot, a handle that was extended): their
// `bytes` are capacities, and no consumer reads them for a length.  caster: the vbm25_caster whose slot the handle is (NULL: owned).
struct vbm25_documents {
    int device = 0;
    uint32_t n_docs = 0;
    uint64_t n_elements = 0;
    bool has_payload = false;
    const void *caster = nullptr;
    bool in_flight = false;  // a caster's slot between the submit that takes it and its collect: the arrays are being written
    vbm25::HbmArray d_start, d_key, d_tf, d_length, d_fieldnorm, d_payload;
};

namespace vbm25 {

// The encode of flush.hip, everything left in HBM.  Lengths on the host (doc_len) or the device (dev_len); payloads on the host
// (doc_payload), the device (dev_payload) or neither (synthetic ctids); the mappings, sorted by (token, document), on the host
// (post_doc / post_tf) or the device (dev_doc / dev_tf); term_key and term_start on the host.
// The bytes the calling thread's last build_device_core copied over the host link: [0] host -> device, [1] device -> host
void encode_link_bytes(double out2[2]);
int build_device_core(int device, double k1, double b, uint32_t n_docs, const uint32_t *doc_len, const uint32_t *dev_len,
                      const uint16_t *doc_payload, const uint16_t *dev_payload, uint32_t n_terms, const uint8_t *term_key,
                      const uint64_t *term_start, const uint32_t *post_doc, const uint32_t *post_tf, const uint32_t *dev_doc,
                      const uint32_t *dev_tf, std::unique_ptr<vbm25_device_segment> &out);

// What vbm25_index_maintain reads of an index (index.hip fills it in, csrc/maintain.hip compacts): the block metadata, the blob,
// term_first_block and the payloads in HBM, the keys on the host
struct MaintainSource {
    int device;
    double k1, b;
    uint32_t n_docs, n_terms, n_blocks;
    const uint8_t *term_key;           // host, n_terms x 16
    const uint32_t *term_first_block;  // device, n_terms + 1
    const uint4 *blk_meta;             // device, per block (min_doc, max_doc, off8, n | meta_doc << 8 | meta_tf << 16 | wand_fn << 24)
    const uint8_t *blob;               // device
    const uint16_t *doc_payload;       // device, n_docs x 3
};
// The compaction's inputs: the host arrays vbm25_index_maintain takes (sealed_deleted, growing), or -- dev != NULL, the host ones are
// then not looked at -- a handle whose planes the kernels read in place (vbm25_index_maintain_device)
struct MaintainInput {
    const uint64_t *sealed_deleted;
    const vbm25_growing_desc *growing;
    const vbm25_device_vacuum *dev;
};
int maintain_device(const MaintainSource &src, const MaintainInput &in, uint32_t *relabel, vbm25_device_segment **out);

// vbm25_filter_remap's device half (csrc/maintain.hip: the relabel is the compaction's).  bits: the old filter's n_bitmaps x
// ceil(n_docs / 64) sealed words; grow_bits: its growing words, bitmap i at word i grow_stride (not read when n_grow is 0); both on
// `device`, as is out: n_bitmaps x ceil(new_n_docs / 64) words, written only when the kept sealed and the live growing documents
// number new_n_docs (else VBM25_ERR_INVALID).  del: the remap's deletion inputs, see RemapDeletions.
// The deletion inputs of the remap: the host arrays vbm25_filter_remap takes (sealed_deleted: NULL or ceil(n_docs / 64) words;
// growing_deleted: NULL or n_grow bytes), or -- dev != NULL, the host ones are then not looked at -- a handle on the filter's device
// whose words and bytes are read in place (vbm25_filter_remap_device; its n_sealed and n_grow are the caller's n_docs and n_grow)
struct RemapDeletions {
    const uint64_t *sealed_deleted;
    const uint8_t *growing_deleted;
    const vbm25_device_vacuum *dev;
};
int filter_remap_device(int device, uint32_t n_bitmaps, uint32_t n_docs, const void *bits, uint32_t n_grow, const RemapDeletions &del,
                        const void *grow_bits, uint32_t grow_stride, uint32_t new_n_docs, void *out);

}  // namespace vbm25

#endif
