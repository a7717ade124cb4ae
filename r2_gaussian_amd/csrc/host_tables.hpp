// host_tables.hpp -- the small host-side tables every forward chain keeps: a fixed-capacity LRU table, the "environment on first use,
// then a control call" switch, and the read-out of a block of statistics counters.  Nothing here knows HIP: a plain C++17 program can
// include it (tests/host_tables_main.cpp does).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdlib>

namespace r2 {

struct NoEvict {
    template <class Key, class Value> void operator()(const Key &, Value &) const {}
};

// Up to N (key, value) entries; a lookup makes its entry the most recently used, an insertion into the full table replaces the least
// recently used one.  on_evict(key, value) runs for an entry that is replaced and for every entry at clear() (and destruction):
// the place to free what the value owns.  Pointers to values stay valid until their entry is evicted.
// NOT an instance of this, on purpose: depth_order.hip's hint history g_hints[2][4].  Its age advances when a hint is UPDATED, not when
// it is looked up, and its `fresh` rule hangs on that clock; as an LruTable it would evict other hints than it does.
template <class Key, class Value, size_t N, class OnEvict = NoEvict>
class LruTable {
public:
    struct Entry { Key key; Value value; unsigned long long used; };
    explicit LruTable(OnEvict on_evict = OnEvict()) : on_evict_(on_evict) {}
    LruTable(const LruTable &) = delete;
    LruTable &operator=(const LruTable &) = delete;
    ~LruTable() { clear(); }

    Value *find(const Key &key)
    {
        for (Entry *e = begin(); e != end(); ++e)
            if (e->key == key) { e->used = ++tick_; return &e->value; }
        return nullptr;
    }
    // a new entry's value is Value()
    Value *find_or_insert(const Key &key)
    {
        if (Value *v = find(key)) return v;
        Entry *e = end();
        if (n_ < N) {
            ++n_;
        } else {
            e = begin();
            for (Entry *o = begin(); o != end(); ++o)
                if (o->used < e->used) e = o;
            on_evict_(e->key, e->value);
        }
        *e = Entry{key, Value(), ++tick_};
        return &e->value;
    }
    void clear()
    {
        for (Entry *e = begin(); e != end(); ++e) on_evict_(e->key, e->value);
        n_ = 0;
    }
    size_t size() const { return n_; }
    Entry *begin() { return e_; }
    Entry *end() { return e_ + n_; }

private:
    Entry e_[N] = {};
    size_t n_ = 0;
    unsigned long long tick_ = 0;
    OnEvict on_evict_;
};

// A process-wide on/off mode: the environment variable decides at first use, a control call (set) overrides it at any time.
// Default on: only a value starting with '0' switches off; default off: only a value starting with '1' switches on.
class EnvSwitch {
public:
    constexpr EnvSwitch(const char *variable, bool default_on) : variable_(variable), default_on_(default_on) {}
    bool on()
    {
        int m = mode_.load(std::memory_order_relaxed);
        if (m < 0) {
            const char *e = getenv(variable_);
            const int want = default_on_ ? !(e && e[0] == '0') : (e && e[0] == '1');
            // several threads may get here at once, or a set() may have come in between: the first to install its answer wins
            int expected = -1;
            mode_.compare_exchange_strong(expected, want, std::memory_order_relaxed);
            m = mode_.load(std::memory_order_relaxed);
        }
        return m == 1;
    }
    void set(int mode)   // 0 / 1; anything else is ignored (the control calls give other values other meanings)
    {
        if (mode == 0 || mode == 1) mode_.store(mode, std::memory_order_relaxed);
    }

private:
    const char *variable_;
    bool default_on_;
    std::atomic<int> mode_{-1};   // -1: not decided yet
};

// out[i] = counters[i] for i < min(count, n_out) (out may be null); reset: every one of the `count` counters back to 0
inline void stats_read(std::atomic<long long> *counters, int count, long long *out, int n_out, int reset)
{
    for (int i = 0; i < count; ++i) {
        if (out && i < n_out) out[i] = counters[i].load(std::memory_order_relaxed);
        if (reset) counters[i].store(0, std::memory_order_relaxed);
    }
}

}  // namespace r2
