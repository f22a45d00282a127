// The owning handle of the host side (insilicoseq_amd/csrc/iss_own.h) with a counting release; built and run by test_own_host.py
// under the address and undefined-behaviour sanitizers.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "iss_own.h"

static int g_released = 0;
static void counting_free(void *p) {
    ++g_released;
    free(p);
}
using Buf = iss_own::Owned<int, counting_free>;

static int *fresh(int n = 4) { return static_cast<int *>(malloc(sizeof(int) * (size_t)n)); }

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct Two {
    Buf a, b;
    int cap = 0;
};
struct Slots {
    Buf d[2][2];
    int cap = 0;
};
static int first_of(const int *p) { return p[0]; }

int main() {
    {   // empty construction
        Buf e;
        CHECK(!e && e.get() == nullptr);
    }
    CHECK(g_released == 0);
    {   // move construction: the source is empty, one release
        Buf a(fresh());
        int *raw = a;
        Buf b(std::move(a));
        CHECK(!a && b.get() == raw);
    }
    CHECK(g_released == 1);
    {   // move assignment releases the old target; self-assignment releases nothing
        Buf a(fresh()), b(fresh());
        int *raw = a;
        b = std::move(a);
        CHECK(g_released == 2 && !a && b.get() == raw);
        Buf &same = b;
        b = std::move(same);
        CHECK(g_released == 2 && b.get() == raw);
    }
    CHECK(g_released == 3);
    {   // reset twice releases once; release() gives the pointer up
        Buf a(fresh());
        a.reset();
        a.reset();
        CHECK(g_released == 4 && !a);
        Buf b(fresh());
        int *raw = b.release();
        CHECK(!b);
        free(raw);
    }
    CHECK(g_released == 4);
    {   // a vector of structs with two handles each, pushed by move
        std::vector<Two> v;
        for (int i = 0; i < 100; ++i) {
            Two t;
            t.a.reset(fresh());
            t.b.reset(fresh());
            t.cap = i;
            v.push_back(std::move(t));
        }
        CHECK(g_released == 4 && v[99].cap == 99 && v[0].a && v[0].b);
    }
    CHECK(g_released == 204);
    {   // a struct with an array of handles assigned {}: each is released, the capacity goes with them
        Slots s;
        for (auto &row : s.d) for (auto &h : row) h.reset(fresh());
        s.cap = 7;
        s = {};
        CHECK(g_released == 208 && s.cap == 0 && !s.d[1][1]);
    }
    CHECK(g_released == 208);
    {   // conversion to T* and pointer arithmetic
        int *raw = fresh(8);
        for (int i = 0; i < 8; ++i) raw[i] = 10 + i;
        Buf a(raw);
        int *p = a;
        const int *view = a + 3;
        CHECK(p == raw && view == raw + 3 && a[5] == 15 && *(a + 1) == 11 && first_of(a) == 10 && (a ? 1 : 0) == 1);
    }
    CHECK(g_released == 209);
    printf("own ok: %d releases\n", g_released);
    return 0;
}
