// Stand-alone check of r2_gaussian_amd/csrc/host_tables.hpp (built and run by test_host_tables_cpu.py with the address and
// undefined-behaviour sanitizers): the LRU table, the environment switch, the statistics read-out.  Exit status 0 = all held.
#include "../r2_gaussian_amd/csrc/host_tables.hpp"

#include <cstdio>
#include <vector>

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

struct Record {
    std::vector<int> *log;
    void operator()(const int &key, int &) const { log->push_back(key); }
};

int main()
{
    using namespace r2;
    {   // ---- LruTable
        std::vector<int> evicted;
        LruTable<int, int, 4, Record> t(Record{&evicted});
        CHECK(t.find(7) == nullptr);
        for (int k = 0; k < 4; ++k) *t.find_or_insert(k) = 10 * k;
        CHECK(t.size() == 4 && evicted.empty());
        for (int k = 0; k < 4; ++k) CHECK(t.find(k) && *t.find(k) == 10 * k);      // an inserted key is found
        CHECK(t.find_or_insert(2) == t.find(2) && *t.find(2) == 20 && evicted.empty());   // ... and found again, not re-inserted
        // use order, oldest first, is now 0 1 3 2; touching 0 makes 1 the least recently used
        CHECK(t.find(0) != nullptr);
        int *v = t.find_or_insert(4);
        CHECK(v && *v == 0);                                                        // a new entry's value is Value()
        CHECK(evicted == std::vector<int>{1});                                      // exactly the least recently used entry went
        CHECK(t.size() == 4 && t.find(1) == nullptr);
        CHECK(t.find(0) && *t.find(0) == 0 && t.find(2) && t.find(3) && t.find(4)); // the entry touched by find survived
        // order: 0 2 3 4 (the finds above, left to right) -> the next two evictions take 0, then 2
        t.find_or_insert(5);
        t.find_or_insert(6);
        CHECK((evicted == std::vector<int>{1, 0, 2}));                              // once per evicted entry
        evicted.clear();
        t.clear();
        CHECK(evicted.size() == 4 && t.size() == 0);                                // once per remaining entry at clear()
        int seen[7] = {0};
        for (int k : evicted) ++seen[k];
        CHECK(seen[3] == 1 && seen[4] == 1 && seen[5] == 1 && seen[6] == 1);
        CHECK(t.find(3) == nullptr);
        evicted.clear();
        t.find_or_insert(9);
    }   // destruction clears: one more call
    {
        std::vector<int> evicted;
        { LruTable<int, int, 2, Record> t(Record{&evicted}); t.find_or_insert(1); }
        CHECK(evicted == std::vector<int>{1});
        LruTable<int, int, 2> plain;   // no callable
        plain.find_or_insert(1); plain.find_or_insert(2); plain.find_or_insert(3);
        CHECK(plain.size() == 2 && !plain.find(1) && plain.find(2) && plain.find(3));
    }
    {   // ---- EnvSwitch
        unsetenv("R2_TEST_SWITCH");
        EnvSwitch on_default("R2_TEST_SWITCH", true), off_default("R2_TEST_SWITCH", false);
        CHECK(on_default.on() && !off_default.on());                                // variable unset: the default
        setenv("R2_TEST_SWITCH", "0", 1);
        EnvSwitch off_by_env("R2_TEST_SWITCH", true);
        CHECK(!off_by_env.on());                                                    // variable set to 0: off
        CHECK(on_default.on());                                                     // (decided at first use, not re-read)
        off_by_env.set(1);
        CHECK(off_by_env.on());                                                     // set(1) overrides the environment
        off_by_env.set(2);
        CHECK(off_by_env.on());                                                     // set(2) is ignored
        off_by_env.set(0);
        off_by_env.set(-1);
        CHECK(!off_by_env.on());
        EnvSwitch early("R2_TEST_SWITCH", true);
        early.set(1);
        CHECK(early.on());                                                          // a set() before the first use holds too
        setenv("R2_TEST_SWITCH", "1", 1);
        EnvSwitch on_by_env("R2_TEST_SWITCH", false);
        CHECK(on_by_env.on());
    }
    {   // ---- stats_read
        std::atomic<long long> c[3];
        for (int i = 0; i < 3; ++i) c[i].store(i + 1);
        long long out[3] = {-1, -1, -1};
        stats_read(c, 3, out, 2, 0);
        CHECK(out[0] == 1 && out[1] == 2 && out[2] == -1 && c[2].load() == 3);
        stats_read(c, 3, nullptr, 0, 1);
        CHECK(c[0].load() == 0 && c[1].load() == 0 && c[2].load() == 0);
    }
    if (g_failed == 0) printf("host tables ok\n");
    return g_failed ? 1 : 0;
}
