// owned.h -- the owners of what a handle keeps between calls: one allocation, a list of allocations, an id table.  Each is templated on an allocator trait
//   static Status alloc(void** out, size_t bytes);      Status() is success (an int, a hipError_t)
//   static void release(void* p);
// is non-copyable and movable, and releases what it holds on destruction.  No policy lives here: a caller that grows a buffer says how large.  Standard C++ only:
// a stand-alone host program can include it (tests/host/owned_main.cpp); owned_hip.h names the HIP allocators.
#pragma once
#include "record_locks.h"
#include <cstddef>
#include <utility>
#include <vector>

template <class Alloc> using OwnedStatus = decltype(Alloc::alloc(nullptr, 0));

// one allocation and its capacity in bytes
template <class Alloc> class Owned {
    void* p_ = nullptr; size_t cap_ = 0;
public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~Owned() { reset(); }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    // at least `need` bytes.  Enough already: same pointer, contents kept.  Otherwise the old allocation is released FIRST (the two never coexist), then `want`
    // bytes are requested: the contents are lost, and the owner stays empty if the request fails
    OwnedStatus<Alloc> room(size_t need, size_t want)
    {
        if (need <= cap_) return OwnedStatus<Alloc>();
        reset();
        const OwnedStatus<Alloc> st = Alloc::alloc(&p_, want);
        if (st != OwnedStatus<Alloc>()) { p_ = nullptr; return st; }
        cap_ = want;
        return st;
    }
    OwnedStatus<Alloc> room(size_t need) { return room(need, need); }         // grown to exactly what is asked
    void reset() { if (p_) Alloc::release(p_); p_ = nullptr; cap_ = 0; }
};

// allocations released together, the latest first
template <class Alloc> class OwnedList {
    std::vector<void*> v_;
public:
    OwnedList() = default;
    OwnedList(const OwnedList&) = delete;
    OwnedList& operator=(const OwnedList&) = delete;
    OwnedList(OwnedList&& o) noexcept { v_.swap(o.v_); }
    OwnedList& operator=(OwnedList&& o) noexcept { if (this != &o) { release(0); v_.swap(o.v_); } return *this; }
    ~OwnedList() { release(0); }
    size_t size() const { return v_.size(); }
    // n elements of T (at least one); *out is written on success only
    template <class T> OwnedStatus<Alloc> add(T** out, size_t n)
    {
        v_.reserve(v_.size() + 1);
        void* p = nullptr;
        const OwnedStatus<Alloc> st = Alloc::alloc(&p, (n ? n : 1) * sizeof(T));
        if (st != OwnedStatus<Alloc>()) return st;
        v_.push_back(p); *out = static_cast<T*>(p);
        return st;
    }
    // all but the first `keep` allocations go
    void release(size_t keep) { while (v_.size() > keep) { Alloc::release(v_.back()); v_.pop_back(); } }
};

// a Table {keys, vals, mask} (device_util.h: CorbIdTable) that owns its memory: one allocation of keys | values | `tail` bytes of the owner's.  It is a Table:
// what reads one reads this
template <class Alloc, class Table> class OwnedTable : public Table {
    Owned<Alloc> mem_;
    void view(size_t cap)
    {
        char* m = mem_.template as<char>();
        this->keys = reinterpret_cast<decltype(this->keys)>(m); this->vals = m ? reinterpret_cast<decltype(this->vals)>(m + cap * 8) : nullptr; this->mask = m ? (unsigned int)(cap - 1) : 0;
    }
public:
    OwnedTable() : Table{nullptr, nullptr, 0} {}
    OwnedTable(const OwnedTable&) = delete;
    OwnedTable& operator=(const OwnedTable&) = delete;
    OwnedTable(OwnedTable&& o) noexcept : Table(o), mem_(std::move(o.mem_)) { o.view(0); }
    OwnedTable& operator=(OwnedTable&& o) noexcept { if (this != &o) { mem_ = std::move(o.mem_); Table::operator=(o); o.view(0); } return *this; }
    // a table of `cap` entries (a power of two) replaces whatever was held
    OwnedStatus<Alloc> own(size_t cap, size_t tail)
    {
        mem_.reset();
        const OwnedStatus<Alloc> st = mem_.room(cap * 12 + tail);
        view(cap);
        return st;
    }
    // holds at least `entries` ids (record_locks.h: id_table_capacity); it only grows, and a table that grows loses its contents
    OwnedStatus<Alloc> room(long long entries)
    {
        const size_t cap = id_table_capacity(entries);
        return this->keys && (size_t)this->mask + 1 >= cap ? OwnedStatus<Alloc>() : own(cap, 0);
    }
    void reset() { mem_.reset(); view(0); }
};
