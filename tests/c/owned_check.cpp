// Host check of csrc/owned.hpp's handle logic against a counting stub allocator; no HIP, no GPU.  Stand-alone:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I minigpt4.cpp_amd/csrc tests/c/owned_check.cpp -o owned_check && ./owned_check
// (any C++17 compiler does: the header is included with MG4_OWNED_NO_HIP).  AddressSanitizer reports a double release or a leak of the stub's blocks; the counters
// below say the same in plain numbers.  Exit status 0 and "owned_check ok" = every check held.
#define MG4_OWNED_NO_HIP
#include "owned.hpp"

#include <cstdio>
#include <cstdlib>
#include <stdexcept>

static int g_live = 0, g_calls = 0, g_acquired = 0, g_released = 0, g_fail_at = -1;   // g_fail_at: the call of acquire (counted from 0) that throws
struct Stub {
    static void *acquire(size_t bytes) {
        if (g_calls++ == g_fail_at) throw std::runtime_error("stub: out of memory");
        g_acquired++; g_live++;
        return malloc(bytes ? bytes : 1);
    }
    static void release(void *p) noexcept { g_released++; g_live--; free(p); }
};
template <typename T> using H = mg4::Owned<T, Stub>;
static_assert(sizeof(H<int>) == sizeof(int *), "one pointer wide");

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "owned_check: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// the engine's pattern for a feature's buffers (Engine::beam_alloc ...): locals first, then moved into the members
struct Feature {
    H<int> a; H<float> b; H<char> c; H<int> d;
    void alloc() { H<int> la(16); H<float> lb(16); H<char> lc(16); H<int> ld(16); a = std::move(la); b = std::move(lb); c = std::move(lc); d = std::move(ld); }
    bool none() const { return !a && !b && !c && !d; }
    bool all() const { return a && b && c && d; }
};

int main() {
    {   // construction, typed access, destruction
        H<int> h(4 * sizeof(int));
        CHECK(h && g_live == 1);
        h[3] = 7; CHECK(h.get()[3] == 7 && *(h + 3) == 7 && h.as<unsigned>()[3] == 7u);
        H<int> empty;
        CHECK(!empty && empty.get() == nullptr);
    }
    CHECK(g_live == 0 && g_acquired == 1 && g_released == 1);
    {   // move construction and move assignment (onto an empty handle, onto a full one, onto itself)
        H<int> a(8);
        int *raw = a.get();
        H<int> b(std::move(a));
        CHECK(!a && b.get() == raw && g_live == 1);
        H<int> c;
        c = std::move(b);
        CHECK(!b && c.get() == raw && g_live == 1);
        H<int> d(8);
        CHECK(g_live == 2);
        d = std::move(c);                                                   // d's own block is released, not leaked
        CHECK(!c && d.get() == raw && g_live == 1);
        H<int> &self = d;
        d = std::move(self);
        CHECK(d.get() == raw && g_live == 1);
    }
    CHECK(g_live == 0 && g_acquired == g_released);
    {   // reset, double reset, abandon
        H<int> a(8);
        a.reset(); CHECK(!a && g_live == 0);
        a.reset(); CHECK(!a && g_live == 0 && g_acquired == g_released);
        H<int> b(8);
        int *raw = b.get();
        const int released = g_released;
        b.abandon();                                                        // leaked on purpose: the handle forgets it, nothing is released
        CHECK(!b && g_released == released && g_live == 1);
        b.reset(); CHECK(g_released == released);
        Stub::release(raw);                                                 // (the check's own clean-up)
        H<int> x(8), y(8);
        mg4::reset_all(x, y); CHECK(!x && !y && g_live == 0);
        H<int> u(8), v(8);
        int *ru = u.get(), *rv = v.get();
        mg4::abandon_all(u, v); CHECK(!u && !v && g_live == 2);
        Stub::release(ru); Stub::release(rv);
    }
    CHECK(g_live == 0 && g_acquired == g_released);
    {   // a group of four whose third allocation fails: nothing stays allocated, the members stay empty; the next attempt succeeds
        Feature f;
        g_fail_at = g_calls + 2;
        bool threw = false;
        try { f.alloc(); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw && f.none() && g_live == 0);
        g_fail_at = -1;
        f.alloc();
        CHECK(f.all() && g_live == 4);
        // ... and a failure while the members are full leaves them as they were
        g_fail_at = g_calls + 2;
        threw = false;
        try { f.alloc(); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw && f.all() && g_live == 4);
        g_fail_at = -1;
    }
    CHECK(g_live == 0 && g_acquired == g_released);
    printf("owned_check ok: %d acquisitions, %d releases\n", g_acquired, g_released);
    return 0;
}
