// C entry points of libicgvins_host.so: self-tests of the host layer's containers, pools and dense helpers (tests only).
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "tracking_batch.h"
#include "factors.h"
#include "object_pool.h"
#include "solver_detail.h"

using namespace icg;

extern "C" {

// HashOrder (track_table.h) against a real std::unordered_map<ulong, int>: n random distinct keys inserted one by one, the iteration
// orders compared after every `check_every` insertions.  Returns 0 when they always agree, k > 0 = first disagreement after k insertions.
int icgh_hashorder_selftest(uint64_t seed, int n, int check_every, int dense_ids) {
    return HashOrder::selfTest(seed, n, check_every, dense_ids != 0);
}

// The tracker core's container order (tc::order_extend, track_core.h: node list + buckets in scratch memory, batched insertion of the rows
// [n_old, n_rows) — what the stage kernels run) against a real std::unordered_map<ulong, int>: `n_first` rows entered at once into an empty
// frame, then `rounds` times `n_more` further rows appended to the existing order (every extension starts from the stored head / buckets and
// crosses rehashes).  Returns 0 when the iteration orders agree after every step, else the step (1-based) of the first disagreement.
int icgh_core_order_selftest(uint64_t seed, int n_first, int n_more, int rounds) {
    if (n_first < 0 || n_more < 0 || rounds < 0 || n_first + (long) n_more * rounds > tc::MAX_ROWS) return -1;
    std::unique_ptr<tc::Frame> f(new tc::Frame);
    std::unique_ptr<tc::Scratch> X(new tc::Scratch);
    memset(f.get(), 0, sizeof(tc::Frame));
    tc::order_clear(*f);
    std::unordered_map<ulong, int> ref;
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 7;
    ulong id   = seed % 977;
    const uint32_t *ba = TableTracker::bucketsAfterTable();
    auto append = [&](int count) {
        for (int k = 0; k < count; k++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            id += 1 + (x % 5) * ((seed & 1) ? 1 : 131); // dense ids as the id factories hand them out, or scattered ones
            f->row[f->n_rows].id = id;
            ref.emplace(id, f->n_rows);
            f->n_rows++;
        }
    };
    auto same = [&]() {
        int r = f->head;
        for (const auto &kv : ref) {
            if (r < 0 || r != kv.second) return false;
            r = f->next[r];
        }
        return r < 0 && (size_t) f->n_buckets == ref.bucket_count();
    };
    int old = 0;
    append(n_first);
    tc::order_extend(*f, old, ba, *X);
    if (!same()) return 1;
    // the sort form (order_extend_parallel) on a copy of the same rows: same list, same buckets, at every step
    std::unique_ptr<tc::Frame> fp(new tc::Frame);
    memset(fp.get(), 0, sizeof(tc::Frame));
    tc::order_clear(*fp);
    auto mirror = [&]() {
        for (int k = fp->n_rows; k < f->n_rows; k++) fp->row[k].id = f->row[k].id;
        fp->n_rows = f->n_rows;
    };
    auto same_as_parallel = [&]() {
        if (fp->head != f->head || fp->n_buckets != f->n_buckets || fp->magic != f->magic) return false;
        for (int k = 0; k < f->n_rows; k++)
            if (fp->next[k] != f->next[k]) return false;
        for (int b = 0; b < f->n_buckets; b++)
            if (fp->bucket[b] != f->bucket[b]) return false;
        return true;
    };
    mirror();
    tc::order_extend_parallel(*fp, 0, ba, *X);
    if (!same_as_parallel()) return 500;
    for (int r = 0; r < rounds; r++) {
        old = f->n_rows;
        append(n_more);
        tc::order_extend(*f, old, ba, *X);
        if (!same()) return 2 + r;
        mirror();
        tc::order_extend_parallel(*fp, old, ba, *X);
        if (!same_as_parallel()) return 501 + r;
    }
    // and the one-by-one form (order_insert_unique: the path of rows added outside a batch) gives the same list
    std::unique_ptr<tc::Frame> g(new tc::Frame);
    memset(g.get(), 0, sizeof(tc::Frame));
    tc::order_clear(*g);
    vector<int32_t> scratch((size_t) tc::MAX_BUCKETS);
    for (int k = 0; k < f->n_rows; k++) {
        g->row[k].id = f->row[k].id;
        tc::order_insert_unique(*g, ba, scratch.data());
    }
    int a = f->head, b = g->head;
    while (a >= 0 && b >= 0 && a == b) a = f->next[a], b = g->next[b];
    return (a < 0 && b < 0) ? 0 : 1000;
}

// symmetricEigen (factors.h) on a caller's matrix: A is n x n row-major, evals (n) ascending, evecs (n x n row-major, eigenvector k in
// column k).  A test hook: tests/test_host_backend_cpu.py pins the bit patterns of the restructured routine to those of the plain form.
int icgh_symmetric_eigen(int n, const double *A, double *evals, double *evecs) {
    if (n < 0 || (n > 0 && (!A || !evals || !evecs))) return -1;
    std::vector<double> a(A, A + (size_t) n * n), ev, V;
    symmetricEigen(n, a, ev, V);
    if (n) memcpy(evals, ev.data(), sizeof(double) * (size_t) n), memcpy(evecs, V.data(), sizeof(double) * (size_t) n * n);
    return 0;
}

// schurReduceGuarded (marg_m3.h) on a caller's system: H is P x P row-major, the m leading columns are eliminated.  Hp (r x r, r = P - m)
// and bp (r) go IN as well: they are what the function finds in its output arrays and come back as it left them, so a caller sees that a
// refusal touched nothing.  Returns 1 = reduced, 0 = refused (an m-block eigenvalue at or below `guard`), -1 = invalid arguments.
int icgh_schur_reduce_guarded(int P, int m, const double *H, const double *b, double guard, double *Hp, double *bp) {
    if (P < 1 || m < 0 || m >= P || !H || !b || !Hp || !bp) return -1;
    const size_t r = (size_t) (P - m);
    std::vector<double> hp(Hp, Hp + r * r), bpv(bp, bp + r);
    const bool ok = schurReduceGuarded(P, m, H, b, guard, hp, bpv);
    if (hp.size() != r * r || bpv.size() != r) return -1;
    memcpy(Hp, hp.data(), sizeof(double) * r * r), memcpy(bp, bpv.data(), sizeof(double) * r);
    return ok ? 1 : 0;
}

// BlockPool / PoolAllocator (object_pool.h) under cross-thread traffic, for tests: `threads` workers each allocate `iters` blocks of two
// size classes, stamp them, hand every second one to the next worker through a mailbox (freed on a thread other than the allocating one:
// the spill / refill path of the per-thread lists) and free the rest themselves; every block is checked for its stamp before it is freed.
// Returns the number of corrupted blocks (0 = pass), -1 on an internal error.
int icgh_pool_selftest(int threads, int iters) {
    struct Small {
        uint64_t tag, a;
    };
    struct Large {
        uint64_t tag, pad[11];
    };
    if (threads < 1 || iters < 1) return -1;
    std::vector<std::mutex> box_m((size_t) threads);
    std::vector<std::vector<std::pair<void *, int>>> box((size_t) threads); // (block, size class)
    std::atomic<int> bad{0}, live{0};
    auto check_free = [&](void *p, int cls) {
        if (cls == 0) {
            Small *s = static_cast<Small *>(p);
            if (s->tag != (0xabcdef0000000000ull ^ (uint64_t) (uintptr_t) p) || s->a != ~s->tag) bad++;
            PoolAllocator<Small>().deallocate(s, 1);
        } else {
            Large *l = static_cast<Large *>(p);
            if (l->tag != (0x1234560000000000ull ^ (uint64_t) (uintptr_t) p) || l->pad[10] != ~l->tag) bad++;
            PoolAllocator<Large>().deallocate(l, 1);
        }
        live--;
    };
    auto worker = [&](int t) {
        std::vector<std::pair<void *, int>> mine;
        for (int i = 0; i < iters; i++) {
            const int cls = (i + t) & 1;
            void *p;
            if (cls == 0) {
                Small *s = PoolAllocator<Small>().allocate(1);
                s->tag   = 0xabcdef0000000000ull ^ (uint64_t) (uintptr_t) s;
                s->a     = ~s->tag;
                p        = s;
            } else {
                Large *l   = PoolAllocator<Large>().allocate(1);
                l->tag     = 0x1234560000000000ull ^ (uint64_t) (uintptr_t) l;
                l->pad[10] = ~l->tag;
                p          = l;
            }
            live++;
            if (i & 1) {
                std::lock_guard<std::mutex> lock(box_m[(size_t) ((t + 1) % threads)]);
                box[(size_t) ((t + 1) % threads)].emplace_back(p, cls);
            } else {
                mine.emplace_back(p, cls);
            }
            if ((i & 63) == 63) { // drain the mailbox and half of the own blocks (LIFO reuse follows)
                std::vector<std::pair<void *, int>> got;
                {
                    std::lock_guard<std::mutex> lock(box_m[(size_t) t]);
                    got.swap(box[(size_t) t]);
                }
                for (auto &g : got) check_free(g.first, g.second);
                for (size_t k = mine.size() / 2; k < mine.size(); k++) check_free(mine[k].first, mine[k].second);
                mine.resize(mine.size() / 2);
            }
        }
        for (auto &m : mine) check_free(m.first, m.second);
    };
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) th.emplace_back(worker, t);
    for (auto &t : th) t.join();
    for (int t = 0; t < threads; t++)
        for (auto &g : box[(size_t) t]) check_free(g.first, g.second);
    return live.load() == 0 ? bad.load() : -1;
}

// the dense helpers of the window solvers (dense_kernels.cc), for tests: in-place Cholesky solve of A x = b (row-major, lower triangle
// read; A is overwritten with the factor, b with x; -1 = not positive definite) and T (upper triangle) += J^T J, g += J^T r
int icgh_dense_cholesky_solve(int n, double *A, double *b) {
    vector<double> Av(A, A + (size_t) n * n), bv(b, b + n);
    if (!solver_detail::choleskySolve(n, Av, bv)) return -1;
    memcpy(A, Av.data(), sizeof(double) * (size_t) n * n);
    memcpy(b, bv.data(), sizeof(double) * (size_t) n);
    return 0;
}
void icgh_dense_accumulate_jtj(int nr, int nf, const double *J, const double *r, double *T, double *g) {
    solver_detail::accumulateJtJ(nr, nf, J, r, T, g);
}

} // extern "C"
