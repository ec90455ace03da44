// gl355_merkle_tree_*: MerkleTree { leaves, digests, cap } resident in HBM and updated in place (include/gl355.h) -- the access set of
// access_set.rs:25,194-205, whose membership changes cost their dirty paths instead of MerkleTree::new over every member.  This file is the C
// boundary: argument checks, the handle and its memory, host planning (merkle_update_plan.h).  The kernels and their launch code are merkle.hip's.
#include "gl355_internal.h"

using namespace gl355;

extern "C" {

int32_t gl355_merkle_tree_create(gl355_ctx* h, int32_t hasher, const uint64_t* leaves, uint64_t n_leaves, uint32_t leaf_len, uint32_t cap_height,
                                 gl355_merkle_tree** out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!out) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_create: null out");
    *out = nullptr;
    if (hasher != GL355_HASH_POSEIDON && hasher != GL355_HASH_BN254_POSEIDON) return ctx->fail(GL355_E_INVALID_ARG, "unknown hasher");
    if (!leaves || n_leaves == 0 || leaf_len == 0) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_create: empty tree");
    const uint32_t lg = log2_u64(n_leaves);
    if (lg > 40 || (1ull << lg) != n_leaves) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_create: n_leaves must be a power of two");
    if (cap_height > lg) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_create: cap_height > log2(n_leaves)");
    const uint64_t n_cap = 1ull << cap_height, n_dig = 2 * (n_leaves - n_cap);
    gl355_merkle_tree* t = new (std::nothrow) gl355_merkle_tree();
    if (!t) return GL355_E_OOM;
    // one allocation: digests | cap | leaves (the digests first: they move as 16-byte words, and a leaf may be an odd number of words)
    void* p = nullptr;
    const int32_t arc = ctx->alloc(((n_dig + n_cap) * 4 + n_leaves * leaf_len) * 8, &p);
    if (arc != GL355_OK) { delete t; return arc; }
    t->ctx = ctx; t->hasher = hasher; t->n_leaves = n_leaves; t->leaf_len = leaf_len; t->cap_height = cap_height; t->sub_bits = lg - cap_height;
    t->digests = reinterpret_cast<uint64_t*>(p); t->cap = t->digests + n_dig * 4; t->leaves = t->cap + n_cap * 4; t->n_digests = n_dig;
    int32_t rc = GL355_OK;
    const hipMemcpyKind kind = ptr_is_device(leaves) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipError_t e = hipMemcpyAsync(t->leaves, leaves, n_leaves * leaf_len * 8, kind, ctx->stream);
    if (e != hipSuccess) rc = ctx->fail_hip(e, "hipMemcpyAsync(leaves)", __FILE__, __LINE__);
    if (rc == GL355_OK) rc = merkle_build_dev(ctx, hasher, t->leaves, n_leaves, leaf_len, false, 0, cap_height, t->digests, t->cap);
    if (rc == GL355_OK && (e = ctx->wait()) != hipSuccess) rc = ctx->fail_hip(e, "hipStreamSynchronize(merkle_tree_create)", __FILE__, __LINE__);
    if (rc != GL355_OK) { ctx->release(p); delete t; return rc; }
    *out = t;
    return GL355_OK;
}

int32_t gl355_merkle_tree_destroy(gl355_merkle_tree* t) {
    if (!t) return GL355_OK;
    (void)hipSetDevice(t->ctx->device);
    (void)t->ctx->wait();
    t->ctx->release(t->digests);
    delete t;
    return GL355_OK;
}

int32_t gl355_merkle_tree_info(const gl355_merkle_tree* t, uint64_t* n_leaves, uint32_t* leaf_len, uint32_t* cap_height, int32_t* hasher) {
    if (!t) return GL355_E_INVALID_ARG;
    if (n_leaves) *n_leaves = t->n_leaves;
    if (leaf_len) *leaf_len = t->leaf_len;
    if (cap_height) *cap_height = t->cap_height;
    if (hasher) *hasher = t->hasher;
    return GL355_OK;
}

// what every entry below starts with: the tree's device, as CTX_OR_FAIL does for a context
#define TREE_OR_FAIL(t)                                \
    if (!(t)) return GL355_E_INVALID_ARG;              \
    Ctx* ctx = (t)->ctx;                               \
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed")

static int32_t tree_copy_out(Ctx* ctx, uint64_t* dst, const uint64_t* src_dev, uint64_t words) {
    if (words == 0) return GL355_OK;
    GL355_HIP(ctx, ctx->d2h(dst, src_dev, words * 8));
    GL355_HIP(ctx, ctx->wait());
    return GL355_OK;
}

int32_t gl355_merkle_tree_cap(const gl355_merkle_tree* t, uint64_t* cap) {
    TREE_OR_FAIL(t);
    if (!cap) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_cap: null buffer");
    return tree_copy_out(ctx, cap, t->cap, 4ull << t->cap_height);
}

int32_t gl355_merkle_tree_digests(const gl355_merkle_tree* t, uint64_t* digests) {
    TREE_OR_FAIL(t);
    if (!digests && t->n_digests) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_digests: null buffer");
    return tree_copy_out(ctx, digests, t->digests, t->n_digests * 4);
}

static int32_t check_indices(Ctx* ctx, const gl355_merkle_tree* t, const uint64_t* indices, uint64_t n_idx, const char* msg) {
    for (uint64_t j = 0; j < n_idx; j++)
        if (indices[j] >= t->n_leaves) return ctx->fail(GL355_E_INVALID_ARG, msg);
    return GL355_OK;
}

int32_t gl355_merkle_tree_leaves(const gl355_merkle_tree* t, const uint64_t* indices, uint64_t n_idx, uint64_t* leaves) {
    TREE_OR_FAIL(t);
    if (!leaves) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_leaves: null buffer");
    if (!indices) return tree_copy_out(ctx, leaves, t->leaves, t->n_leaves * t->leaf_len);
    GL355_TRY(check_indices(ctx, t, indices, n_idx, "merkle_tree_leaves: index out of range"));
    return merkle_tree_gather_dev(ctx, t, 1, indices, n_idx, leaves);
}

int32_t gl355_merkle_tree_prove_batch(const gl355_merkle_tree* t, const uint64_t* indices, uint64_t n_idx, uint64_t* siblings) {
    TREE_OR_FAIL(t);
    if (n_idx == 0) return GL355_OK;
    if (!indices || (!siblings && t->sub_bits)) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_prove_batch: null buffer");
    GL355_TRY(check_indices(ctx, t, indices, n_idx, "merkle_tree_prove_batch: index out of range"));
    return merkle_tree_gather_dev(ctx, t, 0, indices, n_idx, siblings);
}

int32_t gl355_merkle_tree_update(gl355_merkle_tree* t, const uint64_t* indices, uint64_t n_idx, const uint64_t* new_leaves) {
    TREE_OR_FAIL(t);
    if (n_idx == 0) return GL355_OK;
    if (!indices || !new_leaves) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_update: null buffer");
    GL355_TRY(check_indices(ctx, t, indices, n_idx, "merkle_tree_update: index out of range"));      // before anything is enqueued
    try {
        MerkleUpdatePlan p;
        merkle_update_dedup(indices, n_idx, t->n_leaves, p);
        const bool full = merkle_update_is_full(p.leaves.size(), t->n_leaves, ctx->merkle_update_full_log);
        if (!full) merkle_update_layers(t->sub_bits, t->n_leaves, p);
        return merkle_update_dev(ctx, t, p, new_leaves, n_idx, full);
    } catch (...) {      // a failed host allocation; nothing is thrown across the C boundary
        return ctx->fail(GL355_E_OOM, "merkle_tree_update: out of host memory");
    }
}

}  // extern "C"
