// The bookkeeping of released model blocks and of the slab that the models of one mrbf_fit_batch call share -- host code without a
// HIP call of its own (the device allocator comes in as a functor), so that tools/slab_check.cpp can run it under AddressSanitizer
// on a CPU build.  solve.hip instantiates it with hipMalloc / hipFree.
#pragma once
#include <cstddef>
#include <vector>

namespace mrbf {

struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
};
// One device allocation shared by the models of one mrbf_fit_batch call (batch.hip): every model holds one share, destroy_model drops
// it, and the allocation goes back to the context's pool of released model blocks (or to the device) with the last share.
struct ModelSlab {
    void *p = nullptr;
    size_t bytes = 0;
    int refs = 0;
};

constexpr size_t MODEL_POOL_BLOCKS = 8;
constexpr size_t MODEL_POOL_BYTES = size_t(8) << 30;

// a released block: pooled while the pool holds fewer than eight blocks and 8 GiB, else freed.  A slab is worth more than a single
// model's block: when the pool is full it takes the place of the smallest block that is smaller than it, so that the next batch finds
// it whatever single models were released in between.
template <class Free>
void model_pool_release(std::vector<Buf> &pool, void *p, size_t bytes, bool slab, Free free_fn) {
    if (slab && pool.size() >= MODEL_POOL_BLOCKS) {
        size_t least = 0, held = 0;
        for (size_t i = 0; i < pool.size(); ++i) {
            held += pool[i].bytes;
            if (pool[i].bytes < pool[least].bytes) least = i;
        }
        // (only when the slab then fits under the byte cap: otherwise both would be freed)
        if (pool[least].bytes < bytes && held - pool[least].bytes + bytes <= MODEL_POOL_BYTES) {
            free_fn(pool[least].p);
            pool.erase(pool.begin() + least);
        }
    }
    size_t pooled = 0;
    for (const Buf &b : pool) pooled += b.bytes;
    if (pool.size() < MODEL_POOL_BLOCKS && pooled + bytes <= MODEL_POOL_BYTES) {
        Buf b;
        b.p = p;
        b.bytes = bytes;
        pool.push_back(b);
    } else {
        free_fn(p);
    }
}

// a block of at least `total` bytes: a released one when one fits without wasting more than half of it (the smallest such), else a
// new one (alloc_fn(bytes) -> pointer or nullptr; after a failure the pool is dropped and the allocation tried once more).
// Returns false when there is no memory.
template <class Alloc, class Free>
bool model_pool_acquire(std::vector<Buf> &pool, size_t total, void **p, size_t *bytes, Alloc alloc_fn, Free free_fn) {
    int best = -1;
    for (int i = 0; i < (int)pool.size(); ++i)
        if (pool[i].bytes >= total && pool[i].bytes <= 2 * total && (best < 0 || pool[i].bytes < pool[best].bytes)) best = i;
    if (best >= 0) {
        *p = pool[best].p;
        *bytes = pool[best].bytes;
        pool.erase(pool.begin() + best);
        return true;
    }
    *p = alloc_fn(total);
    if (!*p) {
        for (Buf &b : pool) free_fn(b.p);
        pool.clear();
        *p = alloc_fn(total);
    }
    if (!*p) return false;
    *bytes = total;
    return true;
}

// a model drops its share; true when it was the last one (the caller releases slab->p and deletes the slab)
inline bool slab_drop(ModelSlab *slab) { return --slab->refs == 0; }

}  // namespace mrbf
