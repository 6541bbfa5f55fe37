// Stand-alone host check of the bookkeeping behind mrbf_fit_batch's model storage (morbit.jl_amd/csrc/model_pool.hpp): the pool of
// released model blocks and the shares of a slab, with malloc / free in the place of the device allocator.  Build and run under
// AddressSanitizer (no GPU, no library):
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer tools/slab_check.cpp -o /tmp/slab_check && /tmp/slab_check
// A double free, a leak or a use after free of a block shows as a sanitizer report; the program's own checks print what failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../morbit.jl_amd/csrc/model_pool.hpp"

using namespace mrbf;

static std::set<void *> g_live;  // blocks the "device" has handed out and not got back
static int g_allocs = 0, g_failed = 0;

static void *dev_alloc(size_t bytes) {
    void *p = std::malloc(bytes);
    g_live.insert(p);
    ++g_allocs;
    return p;
}
static void dev_free(void *p) {
    if (!g_live.erase(p)) {
        std::printf("FAIL: block %p freed twice or never allocated\n", p);
        ++g_failed;
        return;
    }
    std::free(p);
}
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_failed;                                           \
        }                                                         \
    } while (0)

struct Model {
    void *block = nullptr;
    size_t block_bytes = 0;
    ModelSlab *slab = nullptr;
};
static void destroy(std::vector<Buf> &pool, Model *M) {  // destroy_model's bookkeeping (solve.hip)
    if (M->block) model_pool_release(pool, M->block, M->block_bytes, false, dev_free);
    if (M->slab && slab_drop(M->slab)) {
        model_pool_release(pool, M->slab->p, M->slab->bytes, true, dev_free);
        delete M->slab;
    }
    delete M;
}
static Model *single(std::vector<Buf> &pool, size_t bytes) {
    Model *M = new Model();
    CHECK(model_pool_acquire(pool, bytes, &M->block, &M->block_bytes, dev_alloc, dev_free));
    static_cast<char *>(M->block)[M->block_bytes - 1] = 1;  // the block is whole
    return M;
}
static std::vector<Model *> batch(std::vector<Buf> &pool, int count, size_t per_model) {
    ModelSlab *S = new ModelSlab();
    CHECK(model_pool_acquire(pool, (size_t)count * per_model, &S->p, &S->bytes, dev_alloc, dev_free));
    std::vector<Model *> out;
    for (int i = 0; i < count; ++i) {
        Model *M = new Model();
        M->slab = S;
        ++S->refs;
        static_cast<char *>(S->p)[(size_t)i * per_model] = 1;
        out.push_back(M);
    }
    return out;
}

int main() {
    std::vector<Buf> pool;
    std::mt19937 rng(1);
    // a batch released in a shuffled order returns ONE block, and only with its last model
    auto a = batch(pool, 64, 1 << 16);
    void *slab_p = a[0]->slab->p;
    std::shuffle(a.begin(), a.end(), rng);
    for (size_t i = 0; i + 1 < a.size(); ++i) destroy(pool, a[i]);
    CHECK(pool.empty() && g_live.count(slab_p));
    static_cast<char *>(slab_p)[5] = 2;  // the last model's storage is still there
    destroy(pool, a.back());
    CHECK(pool.size() == 1 && pool[0].p == slab_p);
    // a second identical batch allocates nothing
    const int allocs = g_allocs;
    auto b = batch(pool, 64, 1 << 16);
    CHECK(g_allocs == allocs && b[0]->slab->p == slab_p && pool.empty());
    // nine single models released while the batch is alive: the pool is full of small blocks
    std::vector<Model *> singles;
    for (int i = 0; i < 9; ++i) singles.push_back(single(pool, 4096 + 256 * i));
    for (Model *M : singles) destroy(pool, M);
    CHECK(pool.size() == MODEL_POOL_BLOCKS);
    // ... and the slab still finds a place (the smallest block makes room), so the third batch allocates nothing either
    for (Model *M : b) destroy(pool, M);
    CHECK(pool.size() == MODEL_POOL_BLOCKS);
    CHECK(std::any_of(pool.begin(), pool.end(), [&](const Buf &x) { return x.p == slab_p; }));
    const int allocs2 = g_allocs;
    auto c = batch(pool, 64, 1 << 16);
    CHECK(g_allocs == allocs2 && c[0]->slab->p == slab_p);
    // a single model's block never displaces anything: the tenth release is freed
    for (Model *M : c) destroy(pool, M);
    Model *extra = single(pool, 1 << 20);
    void *extra_p = extra->block;
    // (fill the pool again first: the acquire above may have taken a block out)
    while (pool.size() < MODEL_POOL_BLOCKS) destroy(pool, single(pool, 3000 + 700 * pool.size()));
    destroy(pool, extra);
    CHECK(!g_live.count(extra_p) || std::any_of(pool.begin(), pool.end(), [&](const Buf &x) { return x.p == extra_p; }));
    // a slab smaller than everything pooled does not displace a larger block
    auto tiny = batch(pool, 2, 512);
    void *tiny_p = tiny[0]->slab->p;
    for (Model *M : tiny) destroy(pool, M);
    CHECK(pool.size() <= MODEL_POOL_BLOCKS);
    CHECK(!g_live.count(tiny_p) || std::any_of(pool.begin(), pool.end(), [&](const Buf &x) { return x.p == tiny_p; }));
    // random traffic: batches and singles created and released in any order; at the end everything is pooled or freed exactly once
    std::vector<Model *> alive;
    for (int it = 0; it < 2000; ++it) {
        const int what = (int)(rng() % 4);
        if (what == 0) {
            for (Model *M : batch(pool, 1 + (int)(rng() % 9), 1024 << (rng() % 4))) alive.push_back(M);
        } else if (what == 1) {
            alive.push_back(single(pool, 2048 + 512 * (rng() % 16)));
        } else if (!alive.empty()) {
            const size_t i = rng() % alive.size();
            destroy(pool, alive[i]);
            alive[i] = alive.back();
            alive.pop_back();
        }
        CHECK(pool.size() <= MODEL_POOL_BLOCKS);
    }
    for (Model *M : alive) destroy(pool, M);
    size_t pooled = 0;
    for (const Buf &x : pool) {
        CHECK(g_live.count(x.p));
        pooled += x.bytes;
    }
    CHECK(g_live.size() == pool.size() && pooled <= MODEL_POOL_BYTES);
    for (const Buf &x : pool) dev_free(x.p);  // what mrbf_shutdown does
    CHECK(g_live.empty());
    std::printf(g_failed ? "slab_check: %d check(s) FAILED\n" : "slab_check: ok (%d allocations)\n", g_failed ? g_failed : g_allocs);
    return g_failed ? 1 : 0;
}
