"""The speculation history of the forward (svg-ir_amd/csrc/workload_history.hpp), checked on the host: a small program compiled against
the header with g++ asserts each of its rules with exact numbers."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include "workload_history.hpp"
using namespace svgir;
static int bad = 0;
#define EQ(a, b) do { long long x_ = (long long)(a), y_ = (long long)(b); \
    if (x_ != y_) { std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #a, x_, y_); bad++; } } while (0)
static CapKey key(int P, int W = 256, int scope = 0) { return CapKey{0, W, 256, P, 4, 52, 1, scope}; }
static int guess_R(WorkloadHistory& h, const CapKey& k) { long long s = 0; return h.guess(k, &s); }
static long long guess_slots(WorkloadHistory& h, const CapKey& k) { long long s = 0; h.guess(k, &s); return s; }

int main() {
    {   // instance counts: the largest recent sample, scaled to the caller's Gaussian count (+1 when scaled), at most 4 x the largest raw one
        WorkloadHistory h;
        EQ(guess_R(h, key(1000)), 0);                 // nothing seen
        h.record_R(key(1000), 4000);
        h.record_R(key(1000), 3000);
        EQ(guess_R(h, key(1000)), 4000);              // same P: unscaled
        EQ(guess_R(h, key(1500)), 6001);              // 4000 * 1.5 + 1
        EQ(guess_R(h, key(500)), 2001);               // 4000 * 0.5 + 1
        EQ(guess_R(h, key(2000)), 8001);              // 2 x P: still the same model
        EQ(guess_R(h, key(2100)), 0);                 // more than 2 x P: another model
        EQ(guess_R(h, key(499)), 0);
        EQ(guess_R(h, key(1000, 512)), 0);            // another image size
        for (int i = 0; i < 8; i++) h.record_R(key(1000), 100 + i);
        EQ(guess_R(h, key(1000)), 107);               // the last eight samples only
    }
    {   // the entry follows its model's Gaussian count; scaled samples are clamped to 4 x the largest raw one
        WorkloadHistory h;
        h.record_R(key(1000), 100);
        h.record_R(key(2000), 0);
        h.record_R(key(4000), 0);
        EQ(guess_R(h, key(1000)), 0);                 // (the entry's P is now 4000)
        EQ(guess_R(h, key(8000)), 400);               // 100 * 8 + 1 = 801, clamped to 4 * 100
        EQ(guess_R(h, key(4000)), 400);               // 100 * 4 + 1 = 401, clamped
        EQ(guess_R(h, key(3000)), 301);               // 100 * 3 + 1
    }
    {   // state slots: -1 until one is seen; scaled like the instance counts, clamped to 4 x raw + 64; the fill follows the latest view
        WorkloadHistory h;
        EQ(guess_slots(h, key(1000)), -1);
        EQ(h.guess_fill(key(1000)), -1);
        h.record_R(key(1000), 10);                   // (an entry without slot samples)
        EQ(guess_slots(h, key(1000)), -1);
        h.record_slots(key(1000), 500, 7);
        EQ(guess_slots(h, key(1000)), 500);
        EQ(guess_slots(h, key(1500)), 751);
        EQ(h.guess_fill(key(1000)), 7);
        h.record_slots(key(1000), 400, -1);          // (no fill reported: the last one stays)
        EQ(h.guess_fill(key(1000)), 7);
        EQ(guess_slots(h, key(1000)), 500);
        h.record_slots(key(1000), 300, 0);
        EQ(h.guess_fill(key(1000)), 0);
        WorkloadHistory c;
        c.record_slots(key(1000), 100, 1);
        c.record_R(key(2000), 1);
        c.record_R(key(4000), 1);
        EQ(guess_slots(c, key(8000)), 464);           // 100 * 8 + 1 = 801, clamped to 4 * 100 + 64
        EQ(guess_slots(c, key(4000)), 401);
    }
    {   // depth-key byte: armed by kTopStreak = 3 views with one common top byte, disarmed by a view whose keys differ
        WorkloadHistory h;
        const uint32_t common = 0x4040u, other = 0x4141u, mixed = 0x4041u, none = 0xff00u;
        EQ(WorkloadHistory::kTopStreak, 3);
        h.record_top(key(1000), common);
        h.record_top(key(1000), common);
        EQ(h.guess_top(key(1000)), -1);
        h.record_top(key(1000), none);               // nothing visible: no information
        EQ(h.guess_top(key(1000)), -1);
        h.record_top(key(1000), common);
        EQ(h.guess_top(key(1000)), 0x40);
        h.record_top(key(1000), common);
        EQ(h.guess_top(key(1000)), 0x40);
        h.record_top(key(1000), mixed);              // a visible key outside the byte: the streak starts over
        EQ(h.guess_top(key(1000)), -1);
        h.record_top(key(1000), common);
        h.record_top(key(1000), common);
        h.record_top(key(1000), other);              // another common byte: a new streak of one
        EQ(h.guess_top(key(1000)), -1);
        h.record_top(key(1000), other);
        h.record_top(key(1000), other);
        EQ(h.guess_top(key(1000)), 0x41);
        EQ(h.guess_top(key(1000, 512)), -1);
    }
    {   // 16 entries, least recently used replaced; a look refreshes an entry
        WorkloadHistory h;
        EQ(WorkloadHistory::kEntries, 16);
        for (int w = 0; w < 16; w++) h.record_R(key(1000, 16 * (w + 1)), w + 1);
        EQ(guess_R(h, key(1000, 16)), 1);             // (workload 0 is now the most recently used)
        h.record_R(key(1000, 16 * 17), 17);          // the 17th workload replaces workload 1
        EQ(guess_R(h, key(1000, 32)), 0);
        EQ(guess_R(h, key(1000, 16)), 1);
        EQ(guess_R(h, key(1000, 48)), 3);
        EQ(guess_R(h, key(1000, 16 * 17)), 17);
        h.record_R(key(1000, 16 * 18), 18);          // the next one replaces workload 3 (0, 2 and 17 were looked at since)
        EQ(guess_R(h, key(1000, 64)), 0);
        EQ(guess_R(h, key(1000, 48)), 3);
    }
    {   // a caller that matches two entries gets the first of them
        WorkloadHistory h;
        h.record_R(key(1000), 1000);
        h.record_R(key(2500), 9000);                 // 2.5 x: an entry of its own
        EQ(guess_R(h, key(2500)), 9000);
        EQ(guess_R(h, key(1600)), 1601);              // within 2 x of both: the first entry (1000 * 1.6 + 1)
    }
    {   // reset by scope; the latest view of a workload
        WorkloadHistory h;
        h.record_R(key(1000, 256, 11), 11);
        h.record_R(key(1000, 256, 12), 12);
        h.record_R(key(1000, 256, 0), 10);
        int vp = -7;
        const int blob = 0;
        EQ(h.last_view(key(1000, 128), &vp) == nullptr, 1);   // (no entry: P untouched)
        EQ(vp, -7);
        h.set_last_view(key(1000), &blob, 1100);
        EQ(h.last_view(key(1000), &vp) == &blob, 1);
        EQ(vp, 1100);
        h.reset(11);
        EQ(guess_R(h, key(1000, 256, 11)), 0);
        EQ(guess_R(h, key(1000, 256, 12)), 12);
        EQ(guess_R(h, key(1000, 256, 0)), 10);
        h.reset(-1);
        EQ(guess_R(h, key(1000, 256, 12)), 0);
        EQ(guess_R(h, key(1000, 256, 0)), 0);
        EQ(h.last_view(key(1000), &vp) == nullptr, 1);
    }
    {   // speculation counters
        WorkloadHistory h;
        int64_t s[WorkloadHistory::kStats];
        h.count(WorkloadHistory::kForwards);
        h.count(WorkloadHistory::kForwards);
        h.count(WorkloadHistory::kRerunTop);
        h.stats(s);
        EQ(WorkloadHistory::kStats, 5);
        EQ(s[0], 2); EQ(s[1], 0); EQ(s[2], 0); EQ(s[3], 1); EQ(s[4], 0);
    }
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
'''


def test_workload_history_rules():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        exe = os.path.join(d, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "svg-ir_amd", "csrc"), os.path.join(d, "t.cpp"),
                        "-o", exe, "-pthread"], check=True, capture_output=True, text=True, timeout=300)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout
