// record_locks_main.cpp -- csrc/record_locks.h on its own (tests/test_record_locks_host.py): the id-table capacity against the six loops it replaced, and the lock
// holder on every combination of owner / stores / map -- what is held, what is free, and (under the thread sanitizer) that four threads naming the stores in
// opposite orders take them in one order.
//   record_locks_main capacity | holder | order
// -DRECORD_LOCKS_ARGUMENT_ORDER: the check of the check.  The holder under test is replaced by a copy that takes the stores in argument order, which the
// sanitizer must report in `order`.
#include "record_locks.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#ifdef RECORD_LOCKS_ARGUMENT_ORDER
struct Holder {
    std::unique_lock<std::mutex> lk_owner, lk_a, lk_b, lk_map;
    void take(std::mutex* owner, std::mutex* store_a, std::mutex* store_b, std::mutex* map)
    {
        if (owner) lk_owner = std::unique_lock<std::mutex>(*owner);
        if (store_a) lk_a = std::unique_lock<std::mutex>(*store_a);
        if (store_b && store_b != store_a) lk_b = std::unique_lock<std::mutex>(*store_b);
        if (map) lk_map = std::unique_lock<std::mutex>(*map);
    }
};
#else
typedef RecordLocks Holder;
#endif

// ---- the six historic loops, copied literally; each is labelled by the file it stood in ----
static unsigned int cap_corb_track(int n) { unsigned int cap = 64; while (cap < 2u * (unsigned int)(n > 0 ? n : 1)) cap <<= 1; return cap; }                    // corb_track.cpp: id_table_capacity
static unsigned int cap_corb_kfinsert(long long entries) { unsigned int cap = 64; while ((long long)cap < 2 * std::max<long long>(entries, 1)) cap <<= 1; return cap; }   // corb_kfinsert.cpp: table_cap
static unsigned int cap_covis_host(int capacity) { unsigned int cap = 64; while (cap < 2u * (unsigned int)capacity) cap <<= 1; return cap; }                       // covis_host.h: CovisCall::begin
static unsigned int cap_corb_store(int kf_n) { unsigned int cap = 64; while (cap < 2u * (unsigned int)(kf_n > 0 ? kf_n : 1)) cap <<= 1; return cap; }             // corb_store.cpp: corb_mp_store_replace
static size_t cap_corb_ba_store(int n_kf) { size_t cap = 64; while (cap < 2 * (size_t)n_kf) cap <<= 1; return cap; }                                               // corb_ba_store.cpp: build_graph
static unsigned int cap_build_index(int n) { const unsigned int cap = cap_corb_track(n); return cap; }                                                             // corb_track.cpp: corb_mp_store_build_index (through id_table_capacity)

static int check_capacity()
{
    std::vector<long long> entries = {0, 1, 2, 31, 32, 33};
    for (int k = 6; k <= 24; k++) for (long long d = -1; d <= 1; d++) entries.push_back((1ll << k) + d);
    int bad = 0;
    for (long long e : entries) {
        const size_t got = id_table_capacity(e);
        const size_t want[6] = {cap_corb_track((int)e), cap_corb_kfinsert(e), cap_covis_host((int)e), cap_corb_store((int)e), cap_corb_ba_store((int)e), cap_build_index((int)e)};
        const char* const name[6] = {"corb_track.cpp", "corb_kfinsert.cpp", "covis_host.h", "corb_store.cpp", "corb_ba_store.cpp", "corb_mp_store_build_index"};
        for (int i = 0; i < 6; i++) if (got != want[i]) { printf("capacity(%lld) = %zu, %s gave %zu\n", e, got, name[i], want[i]); bad++; }
        // the closed statement: a power of two, >= 64, >= 2 * max(entries, 1), and the smallest such
        const size_t need = 2 * (size_t)std::max<long long>(e, 1);
        const bool closed = (got & (got - 1)) == 0 && got >= 64 && got >= need && (got == 64 || got / 2 < need);
        if (!closed) { printf("capacity(%lld) = %zu is not the smallest power of two >= 64 and >= %zu\n", e, got, need); bad++; }
    }
    printf("capacity: %zu inputs, %d mismatches\n", entries.size(), bad);
    return bad ? 1 : 0;
}

// ---- the combinations: owner present / absent x (first, second) store x map present / absent ----
struct Mutexes { std::mutex owner, a, b, map; };
struct Combo { bool owner; int first, second; bool map; };              // stores: 0 = null, 1 = A, 2 = B
static std::vector<Combo> combos()
{
    const int pairs[6][2] = {{1, 2}, {2, 1}, {1, 1}, {1, 0}, {0, 2}, {0, 0}};
    std::vector<Combo> c;
    for (int o = 0; o < 2; o++) for (const auto& p : pairs) for (int m = 0; m < 2; m++) c.push_back({o != 0, p[0], p[1], m != 0});
    return c;
}
static std::mutex* store_of(Mutexes& M, int which, bool swapped) { if (which == 0) return nullptr; return ((which == 1) != swapped) ? &M.a : &M.b; }
static void take(Holder& h, Mutexes& M, const Combo& c, bool swapped)
{
    h.take(c.owner ? &M.owner : nullptr, store_of(M, c.first, swapped), store_of(M, c.second, swapped), c.map ? &M.map : nullptr);
}
// which of the four mutexes another thread finds free
static unsigned free_mask(Mutexes& M)
{
    unsigned mask = 0;
    std::thread t([&] {
        std::mutex* all[4] = {&M.owner, &M.a, &M.b, &M.map};
        for (int i = 0; i < 4; i++) if (all[i]->try_lock()) { mask |= 1u << i; all[i]->unlock(); }
    });
    t.join();
    return mask;
}
static int check_holder()
{
    Mutexes M; int bad = 0, n = 0;
    for (const Combo& c : combos()) {
        const unsigned named = (c.owner ? 1u : 0u) | ((c.first == 1 || c.second == 1) ? 2u : 0u) | ((c.first == 2 || c.second == 2) ? 4u : 0u) | (c.map ? 8u : 0u);
        {
            Holder h; take(h, M, c, false);                              // ((A, A) returns: the one mutex is taken once)
            const unsigned free_now = free_mask(M);
            if (free_now != (15u & ~named)) { printf("owner %d stores (%d, %d) map %d: free %x while held, expected %x\n", c.owner, c.first, c.second, c.map, free_now, 15u & ~named); bad++; }
        }
        const unsigned free_after = free_mask(M);
        if (free_after != 15u) { printf("owner %d stores (%d, %d) map %d: free %x after scope exit\n", c.owner, c.first, c.second, c.map, free_after); bad++; }
        n++;
    }
    printf("holder: %d combinations, %d mismatches\n", n, bad);
    return bad ? 1 : 0;
}
// four threads, 2 000 takes each, cycling through the combinations; odd threads name A where even ones name B
static int check_order()
{
    Mutexes M; const std::vector<Combo> cs = combos();
    long long counter = 0;                                               // written under whatever the take holds, and under `guard`, which every thread takes last
    std::mutex guard;
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++) th.emplace_back([&, t] {
        for (int i = 0; i < 2000; i++) {
            Holder h; take(h, M, cs[(size_t)(i + t) % cs.size()], (t & 1) != 0);
            std::lock_guard<std::mutex> g(guard); counter++;
        }
    });
    for (auto& x : th) x.join();
    printf("order: %lld takes\n", counter);
    return counter == 8000 ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s capacity | holder | order\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "capacity")) return check_capacity();
    if (!strcmp(argv[1], "holder")) return check_holder();
    if (!strcmp(argv[1], "order")) return check_order();
    return 2;
}
