// owned_main.cpp -- csrc/owned.h on its own (tests/test_owned_host.py), over an allocator that wraps malloc / free, counts its calls and can be told to fail its
// k-th request.  Every mode ends with the allocator's balance: what was requested was released, once.
//   owned_main room | fail | move | empty | list | table | grow
// -DOWNED_ROOM_FORGETS_RELEASE: the check of the check.  The owner under test is replaced by a copy whose room() forgets to release the old allocation, which
// the address sanitizer's leak check must report in `grow`.
#include "owned.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

struct Fake {
    static int requests, releases, fail_at;                  // fail_at: the request with this number (from 1) fails; 0: none
    static std::set<void*> live;
    static int alloc(void** out, size_t bytes)
    {
        if (++requests == fail_at) { *out = reinterpret_cast<void*>(0x1);  /* a failed request may leave anything there */ return 2; }
        *out = malloc(bytes ? bytes : 1); live.insert(*out);
        return 0;
    }
    static void release(void* p) { releases++; if (!live.erase(p)) { printf("release of %p, which is not live\n", p); releases += 1000; } free(p); }
    static void restart() { requests = releases = fail_at = 0; }
};
int Fake::requests = 0, Fake::releases = 0, Fake::fail_at = 0;
std::set<void*> Fake::live;

#ifdef OWNED_ROOM_FORGETS_RELEASE
struct Mem {
    void* p_ = nullptr; size_t cap_ = 0;
    ~Mem() { if (p_) Fake::release(p_); }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    size_t cap() const { return cap_; }
    int room(size_t need, size_t want) { if (need <= cap_) return 0; const int st = Fake::alloc(&p_, want); if (st) { p_ = nullptr; cap_ = 0; return st; } cap_ = want; return 0; }
};
#else
typedef Owned<Fake> Mem;
#endif
typedef OwnedList<Fake> List;
struct Table { unsigned long long* keys; int* vals; unsigned int mask; };
typedef OwnedTable<Fake, Table> IdTable;

#ifndef OWNED_ROOM_FORGETS_RELEASE
static int bad = 0, checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); bad++; } } while (0)
static int finish(const char* what)
{
    CHECK(Fake::live.empty());
    printf("%s: %d checks, %d mismatches\n", what, checks, bad);
    return bad ? 1 : 0;
}

// need below, equal to and above the capacity
static int check_room()
{
    Fake::restart();
    {
        Mem m;
        CHECK(m.room(100, 128) == 0 && m.cap() == 128 && m.as<char>() != nullptr && Fake::requests == 1 && Fake::releases == 0);
        char* const p = m.as<char>();
        for (int i = 0; i < 128; i++) p[i] = (char)(i * 7);
        CHECK(m.room(64, 4096) == 0 && m.as<char>() == p && m.cap() == 128 && Fake::requests == 1 && Fake::releases == 0);         // below
        CHECK(m.room(128, 4096) == 0 && m.as<char>() == p && m.cap() == 128 && Fake::requests == 1 && Fake::releases == 0);        // equal
        bool kept = true; for (int i = 0; i < 128; i++) kept = kept && p[i] == (char)(i * 7);
        CHECK(kept);
        CHECK(m.room(129, 160) == 0 && m.cap() == 160 && Fake::requests == 2 && Fake::releases == 1 && Fake::live.size() == 1);   // above: one release, one request
        CHECK(m.room(0, 1 << 20) == 0 && m.cap() == 160 && Fake::requests == 2);
        m.reset();
        CHECK(m.as<char>() == nullptr && m.cap() == 0 && Fake::releases == 2);
        CHECK(m.room(0, 64) == 0 && m.as<char>() == nullptr && Fake::requests == 2);                                              // nothing is needed: nothing is asked for
    }
    CHECK(Fake::requests == 2 && Fake::releases == 2);
    return finish("room");
}
// a failed request leaves the owner empty; the old allocation went before the request was made; a later room succeeds
static int check_fail()
{
    Fake::restart();
    {
        Mem m;
        CHECK(m.room(16, 16) == 0);
        Fake::fail_at = 2;
        CHECK(m.room(32, 32) == 2 && m.as<char>() == nullptr && m.cap() == 0 && Fake::releases == 1 && Fake::live.empty());
        CHECK(m.room(8, 8) == 0 && m.as<char>() != nullptr && m.cap() == 8 && Fake::requests == 3);
        Mem first;
        Fake::fail_at = 4;
        CHECK(first.room(8, 8) == 2 && first.as<char>() == nullptr && first.cap() == 0);                                         // the first request of an owner's
        List l; int* a = nullptr; int* b = reinterpret_cast<int*>(0x10);
        CHECK(l.add(&a, 4) == 0 && a != nullptr && l.size() == 1);
        Fake::fail_at = 6;
        CHECK(l.add(&b, 4) == 2 && b == reinterpret_cast<int*>(0x10) && l.size() == 1);                                          // *out is written on success only
        IdTable t;
        CHECK(t.room(10) == 0 && t.keys != nullptr);
        Fake::fail_at = 8;
        CHECK(t.room(1000) == 2 && t.keys == nullptr && t.vals == nullptr && Fake::live.size() == 2);                            // (m's and l's)
        CHECK(t.room(1000) == 0 && t.keys != nullptr && (size_t)t.mask + 1 == id_table_capacity(1000));
    }
    CHECK(Fake::releases == Fake::requests - 4);              // four requests failed
    return finish("fail");
}
static int check_move()
{
    Fake::restart();
    {
        Mem a; CHECK(a.room(16, 16) == 0);
        char* const pa = a.as<char>();
        Mem b(std::move(a));                                                                                                      // construction
        CHECK(a.as<char>() == nullptr && a.cap() == 0 && b.as<char>() == pa && b.cap() == 16 && Fake::releases == 0);
        Mem c; CHECK(c.room(32, 32) == 0);
        c = std::move(b);                                                                                                         // assignment: the target's old allocation goes, once
        CHECK(b.as<char>() == nullptr && b.cap() == 0 && c.as<char>() == pa && c.cap() == 16 && Fake::releases == 1 && Fake::live.size() == 1);
        Mem& same = c; c = std::move(same);
        CHECK(c.as<char>() == pa && Fake::releases == 1);
        Mem empty; c = std::move(empty);
        CHECK(c.as<char>() == nullptr && Fake::releases == 2);

        List l; int* x; CHECK(l.add(&x, 3) == 0 && l.add(&x, 3) == 0);
        List m(std::move(l));
        CHECK(l.size() == 0 && m.size() == 2);
        List n; CHECK(n.add(&x, 1) == 0);
        n = std::move(m);
        CHECK(m.size() == 0 && n.size() == 2 && Fake::releases == 3);

        IdTable t; CHECK(t.room(100) == 0);
        unsigned long long* const keys = t.keys;
        IdTable u(std::move(t));
        CHECK(t.keys == nullptr && t.vals == nullptr && u.keys == keys && u.mask == 255);
        IdTable v; CHECK(v.room(1) == 0);
        v = std::move(u);
        CHECK(u.keys == nullptr && v.keys == keys && v.mask == 255 && reinterpret_cast<char*>(v.vals) == reinterpret_cast<char*>(keys) + 256 * 8 && Fake::releases == 4);
    }
    CHECK(Fake::requests == 7 && Fake::releases == 7);
    return finish("move");
}
static int check_empty()
{
    Fake::restart();
    { Mem m; List l; IdTable t; Mem moved(std::move(m)); m.reset(); l.release(0); t.reset(); }
    CHECK(Fake::requests == 0 && Fake::releases == 0);
    return finish("empty");
}
// add, then release(keep) for keep = 0, 1 and all: the latest go first, the first `keep` stay where they are
static int check_list()
{
    Fake::restart();
    const size_t keeps[3] = {0, 1, 4};
    for (size_t keep : keeps) {
        const int before = Fake::releases;
        List l; double* p[4];
        for (int i = 0; i < 4; i++) { CHECK(l.add(&p[i], (size_t)i) == 0 && p[i] != nullptr); p[i][0] = i; }                      // (0 elements: one)
        CHECK(l.size() == 4);
        l.release(keep);
        CHECK(l.size() == keep && Fake::releases - before == (int)(4 - keep));
        for (size_t i = 0; i < keep; i++) CHECK(Fake::live.count(p[i]) == 1 && p[i][0] == (double)i);
        for (size_t i = keep; i < 4; i++) CHECK(Fake::live.count(p[i]) == 0);
        l.release(keep + 3);
        CHECK(l.size() == keep);
    }
    CHECK(Fake::requests == 12 && Fake::releases == 12);
    return finish("list");
}
// the capacity is id_table_capacity's; the table never shrinks; an equal or smaller request does not reallocate
static int check_table()
{
    Fake::restart();
    std::vector<long long> entries = {0, 1, 31, 32, 33};
    for (int k = 6; k <= 12; k++) for (long long d = -1; d <= 1; d++) entries.push_back((1ll << k) + d);
    int n = 0;
    {
        IdTable t; size_t held = 0;
        for (int pass = 0; pass < 2; pass++)                                         // ascending, then descending: the second pass may change nothing
            for (size_t i = 0; i < entries.size(); i++) {
                const long long e = entries[pass ? entries.size() - 1 - i : i];
                const int before = Fake::requests; unsigned long long* const keys = t.keys;
                CHECK(t.room(e) == 0);
                const size_t cap = (size_t)t.mask + 1, want = id_table_capacity(e);
                if (want > held) { CHECK(cap == want && Fake::requests == before + 1); held = want; }
                else CHECK(cap == held && t.keys == keys && Fake::requests == before);
                CHECK(t.keys != nullptr && reinterpret_cast<char*>(t.vals) == reinterpret_cast<char*>(t.keys) + cap * 8 && Fake::live.size() == 1);
                n++;
            }
        // a fresh table per request holds exactly the capacity; own() replaces whatever is held, with the tail behind the values
        for (long long e : entries) { IdTable f; CHECK(f.room(e) == 0 && (size_t)f.mask + 1 == id_table_capacity(e)); CHECK(f.room(e) == 0 && f.room(e > 0 ? e - 1 : 0) == 0); n++; }
        const int before = Fake::requests;
        CHECK(t.own(64, 256) == 0 && t.mask == 63 && Fake::requests == before + 1 && Fake::live.size() == 1);
        memset(t.keys, 0xFF, 64 * 12 + 256);                                         // (all of it is the table's: the sanitizer watches the bounds)
    }
    CHECK(Fake::requests == Fake::releases);
    printf("table: %d requests\n", n);
    return finish("table");
}
#endif
// what the forgetful copy leaks
static int grow()
{
    Mem m;
    if (m.room(16, 16) || m.room(32, 32) || m.room(64, 64)) return 1;
    printf("grow: capacity %zu\n", m.cap());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s room | fail | move | empty | list | table | grow\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "grow")) return grow();
#ifndef OWNED_ROOM_FORGETS_RELEASE
    if (!strcmp(argv[1], "room")) return check_room();
    if (!strcmp(argv[1], "fail")) return check_fail();
    if (!strcmp(argv[1], "move")) return check_move();
    if (!strcmp(argv[1], "empty")) return check_empty();
    if (!strcmp(argv[1], "list")) return check_list();
    if (!strcmp(argv[1], "table")) return check_table();
#endif
    return 2;
}
