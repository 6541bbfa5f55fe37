// What the many-start chains (sd_batch.hip, normal_batch.hip) share: the arena's bookkeeping, the host blocks of the packed upload and
// of the read-back, and the evaluations of a batch -- model slot j of start p at one of the chain's sites -- grouped by what one eval_fused_batch launch requires, with their
// descriptors and their scratch in the chain's arena.  Every member takes the centre-range split of the single call it stands for
// (eval_nsplit on its own query count) and partial buffers of its own, so the order of every sum is that call's.
#pragma once
#include "small.hpp"

namespace mrbf {
namespace chain {

// the chain's one device arena, counted in doubles: every piece a multiple of 16
struct Arena {
    size_t total = 0;
    size_t take(size_t cnt) {
        const size_t at = total;
        total += (cnt + 15) & ~(size_t)15;
        return at;
    }
};
// a host block of `cnt` T for the upload or the read-back: in the armed pinned block where it fits in 4 MiB, else pageable
template <class T>
struct Block {
    std::vector<T> own;
    T *p = nullptr;
    Block() = default;
    Block(mrbf_ctx *ctx, size_t cnt) {
        p = reinterpret_cast<T *>(cnt * sizeof(T) <= ((size_t)4 << 20) ? pin_take(ctx, cnt * sizeof(T)) : nullptr);
        if (!p) {
            own.resize(cnt);
            p = own.data();
        }
    }
};
using Staging = Block<double>;  // the descent chains count doubles; select_call.hpp counts bytes

constexpr int64_t MAX_GROUP_LAUNCH = 65535;  // blockIdx.z of the evaluation kernels

// one evaluation of the batch: model slot j of start p at `site`, mq query rows
struct Member {
    int site, j;
    int64_t p;
    int group;  // launch group, or -1: eval_model
    const mrbf_model *M;
    int64_t mq;
    bool jac;
    // where the member reads and writes, offsets in doubles from the arena's base: the caller's to set before fill() / launch()
    size_t X = 0, vals = 0, jacs = 0;
    // ... or, with `ext`, buffers outside the arena (mrbf_eval_batch: a caller's device buffers, used in place) by their addresses;
    // vals_at may then be NULL (Jacobians only), jac_at is read where `jac` is set
    bool ext = false;
    const double *X_at = nullptr;
    double *vals_at = nullptr, *jac_at = nullptr;
    const double *x_of(const double *base) const { return ext ? X_at : base + X; }
    double *vals_of(double *base) const { return ext ? vals_at : base + vals; }
    double *jac_of(double *base) const { return !jac ? nullptr : (ext ? jac_at : base + jacs); }
    // scratch (carve): offsets likewise
    size_t Xq = 0, xsq = 0, vpart = 0, gpart = 0;
    int64_t mpad = 0;
    int nsplit = 1, KO = 0;
};
struct Group {
    int site, D, k;
    bool jac;
    KP kp;
    std::vector<size_t> members;
    size_t first;  // index of the group's first descriptor in the device array
};

struct Plan {
    std::vector<Member> mem;
    std::vector<Group> groups;
    size_t n_desc = 0;

    // members are added site by site; a group is (site, kernel and parameters, k, dpad, split or unsplit centre range)
    // (population: a sweep over a population of the PS solver -- EvalHints::population of the single call it stands for)
    void add(const mrbf_ctx *ctx, int site, int64_t p, int j, const mrbf_model *M, int64_t mq, bool jac, bool population = false) {
        Member mb;
        mb.site = site, mb.j = j, mb.p = p, mb.M = M, mb.mq = mq, mb.jac = jac;
        mb.nsplit = eval_nsplit(ctx, mq, (int)((M->n + 63) / 64), false, population);
        mb.group = group_of(ctx, site, M, jac, mb.nsplit > 1);
        if (mb.group >= 0) groups[mb.group].members.push_back(mem.size());
        mem.push_back(mb);
    }
    // the plan of the members `which` of this plan alone, in that order, every one in the places it has here (its inputs and outputs, and
    // the scratch carve() gave it): a later phase of a chain that only some starts take part in
    Plan select(const mrbf_ctx *ctx, const std::vector<size_t> &which) const {
        Plan out;
        for (size_t i : which) {
            Member mb = mem[i];
            mb.group = out.group_of(ctx, mb.site, mb.M, mb.jac, mb.nsplit > 1);
            if (mb.group >= 0) out.groups[mb.group].members.push_back(out.mem.size());
            out.mem.push_back(mb);
        }
        out.close();
        return out;
    }
    // after the last add: the descriptors' places
    void close() {
        n_desc = 0;
        for (Group &G : groups) G.first = n_desc, n_desc += G.members.size();
    }
    size_t desc_doubles() const { return (n_desc * sizeof(EvalDesc) + sizeof(double) - 1) / sizeof(double); }
    // the scratch of every grouped member, in member order
    void carve(Arena &ar) {
        auto take = [&](size_t cnt) { return ar.take(cnt); };
        for (Member &S : mem) {
            if (S.group < 0) continue;
            S.mpad = round_up(S.mq, 64);
            S.KO = outputs_per_pass(S.M->k, S.M->dpad, S.jac);
            S.Xq = take((size_t)S.mpad * S.M->dpad);
            S.xsq = take((size_t)S.mpad);
            S.vpart = take(S.nsplit > 1 ? (size_t)S.nsplit * S.mpad * S.KO * 2 : 0);
            S.gpart = take((S.nsplit > 1 && S.jac) ? (size_t)S.nsplit * S.mpad * S.KO * S.M->dpad : 0);
        }
    }
    // the descriptors (host copy, to be uploaded to the same place of the arena), group by group
    void fill(double *base, EvalDesc *hdesc) const {
        for (const Group &G : groups)
            for (size_t r = 0; r < G.members.size(); ++r) {
                const Member &S = mem[G.members[r]];
                EvalDesc E;
                std::memset(&E, 0, sizeof(E));
                eval_desc_model(E, S.M, S.mq, S.nsplit);
                E.X = S.x_of(base);
                E.Xq = base + S.Xq;
                E.xsq = base + S.xsq;
                if (S.nsplit > 1) {
                    E.vpart = base + S.vpart;
                    E.sapart = E.vpart + (size_t)S.nsplit * S.mpad * S.KO;
                    if (S.jac) E.gpart = base + S.gpart;
                }
                E.vals = S.vals_of(base);
                E.jac = S.jac_of(base);
                std::memcpy(&hdesc[G.first + r], &E, sizeof(E));
            }
    }
    // the evaluations of one site on the ctx stream: its launch groups, then the members the fused kernels do not take
    // (centred: every grouped member's Xq / xsq are filled already -- the PS solver's breeding kernel wrote them)
    int launch(mrbf_ctx *ctx, int site, double *base, const EvalDesc *hdesc, const EvalDesc *ddesc, bool centred = false) const {
        for (const Group &G : groups) {
            if (G.site != site) continue;
            for (size_t r0 = 0; r0 < G.members.size(); r0 += MAX_GROUP_LAUNCH) {
                const int cnt = (int)std::min<size_t>(MAX_GROUP_LAUNCH, G.members.size() - r0);
                MRBF_TRY(eval_fused_batch(ctx, G.kp, G.D, G.k, G.jac, hdesc + G.first + r0, ddesc + G.first + r0, cnt, centred));
            }
        }
        for (const Member &S : mem) {
            if (S.site != site || S.group >= 0) continue;
            MRBF_TRY(eval_model(ctx, S.M, S.mq, S.x_of(base), S.vals_of(base), S.jac_of(base), nullptr));
        }
        return 0;
    }

private:
    int group_of(const mrbf_ctx *ctx, int site, const mrbf_model *M, bool jac, bool split) {
        if (ctx->eval_impl == 1 || !(M->dpad == 64 || M->dpad == 128 || M->dpad == 256)) return -1;
        for (size_t g = 0; g < groups.size(); ++g) {
            const Group &G = groups[g];
            if (G.site == site && G.D == M->dpad && G.k == M->k && G.jac == jac && std::memcmp(&G.kp, &M->kp, sizeof(KP)) == 0) {
                // (the group's kernels either all write partial sums or none does: split and unsplit members launch apart)
                return (int)(g & ~(size_t)1) + (split ? 1 : 0);
            }
        }
        // a new key: its unsplit group, then its split group
        for (int s = 0; s < 2; ++s) {
            Group G;
            G.site = site, G.D = M->dpad, G.k = M->k, G.jac = jac, G.kp = M->kp, G.first = 0;
            groups.push_back(G);
        }
        return (int)groups.size() - 2 + (split ? 1 : 0);
    }
};

}  // namespace chain
}  // namespace mrbf
