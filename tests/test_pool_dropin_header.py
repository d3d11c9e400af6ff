"""The pool extension of the C++ drop-in header (SignalsmithStretch::Pool, processAsync, wait): C++11, clean under -Wall -Wextra,
and bit for bit what plain process() gives.  Compiled against the CPU stand-in and run."""
import os
import subprocess
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = textwrap.dedent(r'''
    #include "signalsmith-stretch/signalsmith-stretch.h"
    #include <cmath>
    #include <cstdio>
    #include <vector>
    using Stretch = signalsmith::stretch::SignalsmithStretch<float>;
    using Wide = signalsmith::stretch::SignalsmithStretch<double>;
    typedef std::vector<std::vector<float>> Buffers;
    typedef std::vector<std::vector<double>> WideBuffers;
    static Buffers signal(int seed, int channels, int offset, int n) {
        Buffers x(channels, std::vector<float>(n));
        for (int c = 0; c < channels; ++c) for (int i = 0; i < n; ++i) x[c][i] = 0.4f*float(std::sin(0.01*(seed + 3)*(i + offset) + 0.5*c)) + 0.1f*float(((i + offset)*7 + seed*13)%97)/97;
        return x;
    }
    int main() {
        const int N = 5, nIn = 400, nOut = 1000; // 2.5x: seeded random time factors
        std::vector<Stretch> pooled, plain;
        for (int s = 0; s < N; ++s) {
            pooled.emplace_back(long(50 + s)); plain.emplace_back(long(50 + s));
            pooled[s].configure(2, 512, 128, s%2 == 1); plain[s].configure(2, 512, 128, s%2 == 1); // two geometries
        }
        Wide widePooled(77L), widePlain(77L);
        widePooled.configure(1, 512, 128); widePlain.configure(1, 512, 128);
        std::vector<Buffers> out(N, Buffers(2, std::vector<float>(nOut))), want(N, Buffers(2, std::vector<float>(nOut)));
        WideBuffers wideIn(1, std::vector<double>(nIn)), wideOut(1, std::vector<double>(nOut)), wideWant(1, std::vector<double>(nOut));
        int step = 0;
        {
            Stretch::Pool pool;
            for (int s = 0; s < N; ++s) pool.add(pooled[s]);
            Wide::Pool widePool;
            widePool.add(widePooled);
            if (pool.members() != N) return 1;
            for (; step < 3; ++step) {
                for (int s = 0; s < N; ++s) pooled[s].processAsync(signal(s, 2, step*nIn, nIn), nIn, out[s], nOut); // (the inputs are temporaries: read at once)
                if (pool.pending() != N) return 2;
                pool.run();
                if (pool.pending() != 0) return 3;
                for (int s = 0; s < N; ++s) { pooled[s].wait(); plain[s].process(signal(s, 2, step*nIn, nIn), nIn, want[s], nOut); }
                for (int s = 0; s < N; ++s) if (out[s] != want[s]) { std::printf("step %d object %d differs\n", step, s); return 4; }
                for (int i = 0; i < nIn; ++i) wideIn[0][i] = 0.3*std::sin(0.02*(i + step*nIn));
                widePooled.processAsync(wideIn, nIn, wideOut, nOut);
                widePooled.wait(); // runs the pool; the doubles are converted back here
                widePlain.process(wideIn, nIn, wideWant, nOut);
                if (wideOut != wideWant) { std::printf("step %d: the double object differs\n", step); return 5; }
            }
            // a copy of a pooled object is an unpooled, independent object with the same state
            pooled[1].processAsync(signal(1, 2, step*nIn, nIn), nIn, out[1], nOut);
            Stretch copy(pooled[1]); // (the pending request runs first)
            if (pool.pending() != 0 || pool.members() != N) return 6;
            pooled[1].wait();
            plain[1].process(signal(1, 2, step*nIn, nIn), nIn, want[1], nOut);
            if (out[1] != want[1]) return 7;
            Buffers copyOut(2, std::vector<float>(nOut));
            copy.process(signal(1, 2, (step + 1)*nIn, nIn), nIn, copyOut, nOut);
            pooled[1].processAsync(signal(1, 2, (step + 1)*nIn, nIn), nIn, out[1], nOut);
            pooled[1].wait();
            if (copyOut != out[1]) return 8;
            plain[1].process(signal(1, 2, (step + 1)*nIn, nIn), nIn, want[1], nOut);
            if (out[1] != want[1]) return 9;
            // a moved pooled object keeps its membership -- and a request that is pending
            pooled[2].processAsync(signal(2, 2, step*nIn, nIn), nIn, out[2], nOut);
            Stretch moved(std::move(pooled[2]));
            if (pool.pending() != 1 || pool.members() != N) return 10;
            moved.wait();
            plain[2].process(signal(2, 2, step*nIn, nIn), nIn, want[2], nOut);
            if (out[2] != want[2]) return 11;
            float *planes[2] = {out[2][0].data(), out[2][1].data()};
            moved.processAsync(signal(2, 2, (step + 1)*nIn, nIn), nIn, planes, nOut);
            pool.run();
            moved.wait();
            plain[2].process(signal(2, 2, (step + 1)*nIn, nIn), nIn, want[2], nOut);
            if (out[2] != want[2]) return 12;
            pool.remove(moved);
            if (pool.members() != N - 1) return 13;
            pooled[2] = std::move(moved); // back into the vector, unpooled now
            // the pool goes out of scope with a request pending: it runs, the members go on unattached
            pooled[0].processAsync(signal(0, 2, step*nIn, nIn), nIn, out[0], nOut);
        }
        pooled[0].wait();
        plain[0].process(signal(0, 2, step*nIn, nIn), nIn, want[0], nOut);
        if (out[0] != want[0]) return 14;
        for (int s = 3; s < N; ++s) { // not in a pool: processAsync is process
            pooled[s].processAsync(signal(s, 2, step*nIn, nIn), nIn, out[s], nOut);
            pooled[s].wait();
            plain[s].process(signal(s, 2, step*nIn, nIn), nIn, want[s], nOut);
            if (out[s] != want[s]) return 15;
        }
        float peak = 0;
        for (int i = 0; i < nOut; ++i) peak = std::fmax(peak, std::fabs(want[0][0][i]));
        std::printf("ok peak %g\n", peak);
        return peak > 1e-3f ? 0 : 16;
    }
''')


def test_pool_through_the_dropin_header(emu, tmp_path):
    src, exe = tmp_path / "pool.cpp", tmp_path / "pool"
    src.write_text(SOURCE)
    emu_dir = os.path.join(ROOT, "tests", "emu")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L" + emu_dir, "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
