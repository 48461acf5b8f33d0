"""The host-side plumbing of `tksm sequence` (csrc/module_stream.h, ChunkReader of csrc/module_log.h) as a stand-alone program under the
thread sanitizer and under the address + undefined-behaviour sanitizers: run as a process of its own, nothing is loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r'''
#include "module_log.h"
#include "module_stream.h"
#include <chrono>
#include <cstdio>
#include <string>
#include <thread>

using namespace tkmod;
struct Item { uint64_t seq = 0; };
static const uint64_t N = 200;
static uint64_t size_of(uint64_t seq) { return (seq * 2654435761u) % 97 + (seq % 5 == 0 ? 0 : 1); }   // pseudo-random, some zero

// 3 producers take numbers 0..N-1 with their tickets and hand them, in ticket order, into a queue of capacity 2; 3 consumers take a
// place for each (and, `turns`, write in their turn into a shared log).  `fail_at`: fail() once that many places are taken.
static int pipeline(bool turns, uint64_t fail_at) {
    BoundedQueue<Item> q(2); Handover turn; BatchOrder order(3, 0);
    uint64_t next = 0;                                        // guarded by the hand-over's take
    std::vector<uint64_t> off(N, ~0ull), seen(N, 0), log;     // log: guarded by the turn
    std::atomic<uint64_t> places{0};
    auto fail = [&] { order.fail(); q.close(); };
    std::vector<std::thread> th;
    for (int p = 0; p < 3; p++) th.emplace_back([&] {
        for (;;) {
            Item it; uint64_t ticket = 0;
            if (!turn.take(ticket, [&] { if (next == N || order.failed()) return false; it.seq = next++; return true; })) return;
            if (it.seq % 7 == 3) std::this_thread::sleep_for(std::chrono::microseconds(200));      // a slow producer: the others wait for its ticket
            turn.hand(ticket, [&] { (void)q.push(std::move(it)); });
        }
    });
    for (int c = 0; c < 3; c++) th.emplace_back([&, c] {
        Item it;
        while (q.pop(it)) {
            if (places.load() >= fail_at) { fail(); continue; }
            uint64_t o = 0;
            if (!order.take_place(0, it.seq, size_of(it.seq), 1, o)) continue;
            places++;
            off[it.seq] = o; seen[it.seq]++;
            if (turns) { if (!order.wait_turn(1, it.seq)) continue; log.push_back(it.seq); order.turn_done(1, true); }
            if (c == 1) std::this_thread::yield();
        }
    });
    if (fail_at >= N) {
        for (auto& t : th) if (&t - th.data() < 3) t.join();
        q.close();                                            // end of input: the consumers take what is queued
        for (auto& t : th) if (t.joinable()) t.join();
        uint64_t sum = 0;
        for (uint64_t s = 0; s < N; s++) {
            if (seen[s] != 1 || off[s] != sum) { std::printf("batch %llu: seen %llu, offset %llu, expected %llu\n", (unsigned long long)s, (unsigned long long)seen[s], (unsigned long long)off[s], (unsigned long long)sum); return 1; }
            sum += size_of(s);
        }
        if (order.bytes(0) != sum || order.reads() != N) return 2;
        if (turns) { if (log.size() != N) return 3; for (uint64_t s = 0; s < N; s++) if (log[s] != s) return 4; }
    } else {
        for (auto& t : th) t.join();                          // fail() was raised while producers and consumers block: everybody returns
        if (!order.failed()) return 5;
        uint64_t o = 0; Finished f;
        if (order.take_place(0, N + 1, 1, 1, o) || order.wait_turn(1, N + 1) || order.wait_host_free(0) || order.next_finished(N + 1, f)) return 6;   // no wait after fail()
    }
    return 0;
}

// The ordered writer: 2 makers (a hand-over that lets one make at a time) feed 3 workers, which fill their host buffer once the writer
// has written their previous batch and announce it; one writer takes the finished batches in batch order until end().
static int ordered_writer() {
    BoundedQueue<Item> q(2); Handover turn(true); BatchOrder order(3, 0);
    uint64_t next = 0; int making = 0;                        // guarded by the hand-over's take, held until the hand-over
    uint64_t host[3] = {~0ull, ~0ull, ~0ull};                 // a worker's buffer: the worker's while free, the writer's while busy
    std::vector<uint64_t> log; bool two_makers = false;
    std::vector<std::thread> makers, workers;
    for (int p = 0; p < 2; p++) makers.emplace_back([&] {
        for (;;) {
            Item it; uint64_t ticket = 0;
            if (!turn.take(ticket, [&] { if (next == N) return false; it.seq = next++; return true; })) return;
            if (making++) two_makers = true;
            if (it.seq % 7 == 3) std::this_thread::sleep_for(std::chrono::microseconds(200));
            turn.hand(ticket, [&] { making--; (void)q.push(std::move(it)); });
        }
    });
    for (int w = 0; w < 3; w++) workers.emplace_back([&, w] {
        Item it;
        while (q.pop(it)) {
            if (!order.wait_host_free(w)) return;
            host[w] = it.seq;
            Finished f; f.worker = w; f.bytes[0] = size_of(it.seq); f.bytes[1] = 2; f.n_reads = 1;
            order.finished(it.seq, f);
        }
    });
    std::thread writer([&] {
        Finished f;
        for (uint64_t s = 0; order.next_finished(s, f); s++) {
            const bool ok = host[f.worker] == s && f.bytes[0] == size_of(s);      // not filled again before it was written
            log.push_back(ok ? s : ~0ull);
            order.written(f, true);
        }
    });
    for (auto& t : makers) t.join();
    order.end(N);
    q.close();
    for (auto& t : workers) t.join();
    writer.join();
    uint64_t sum = 0;
    if (two_makers || log.size() != N) return 1;
    for (uint64_t s = 0; s < N; s++) { if (log[s] != s) return 2; sum += size_of(s); }
    if (order.bytes(0) != sum || order.bytes(1) != 2 * N || order.reads() != N || order.failed()) return 3;
    return 0;
}

// ChunkReader over a read function that returns 1 - 7 bytes at a time == ChunkReader over fread
static int short_reads(const char* path) {
    std::string all;
    for (int m = 0; m < 300; m++) {
        all += "+mol" + std::to_string(m) + "\t" + std::to_string(m % 3) + "\tc=+x;\n";
        for (int l = 0; l < (m == 11 ? 400 : 1 + m % 4); l++) all += "chr1\t" + std::to_string(100 * l) + "\t" + std::to_string(100 * l + 90) + "\t+\t3A,7+\n";
    }
    FILE* f = fopen(path, "wb"); fwrite(all.data(), 1, all.size(), f); fclose(f);
    const uint64_t sizes[] = {64, 4096};
    for (uint64_t b : sizes) {
        ChunkReader plain; plain.in = fopen(path, "rb"); plain.bytes = b;
        ChunkReader custom; custom.bytes = b;
        size_t at = 0; uint32_t r = 12345;
        custom.read = [&](char* dst, size_t n) { r = r * 1664525u + 1013904223u; size_t k = std::min<size_t>({n, 1 + (r >> 16) % 7, all.size() - at}); memcpy(dst, all.data() + at, k); at += k; return k; };
        std::vector<char> p1, p2; std::string got;
        for (;;) {
            const bool m1 = plain.next(p1), m2 = custom.next(p2);
            if (m1 != m2 || (m1 && p1 != p2)) { std::printf("pieces differ at size %llu\n", (unsigned long long)b); return 1; }
            if (!m1) break;
            got.append(p2.begin(), p2.end());
        }
        fclose(plain.in);
        if (got != all) return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (int rc = pipeline(false, N)) { std::printf("places: %d\n", rc); return 1; }
    if (int rc = pipeline(true, N)) { std::printf("turns: %d\n", rc); return 1; }
    if (int rc = pipeline(true, 50)) { std::printf("fail: %d\n", rc); return 1; }
    if (int rc = ordered_writer()) { std::printf("ordered writer: %d\n", rc); return 1; }
    if (int rc = short_reads(argv[1])) { std::printf("short reads: %d\n", rc); return 1; }
    std::puts("ok");
    return 0;
}
'''


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_queue_handover_order_and_chunk_reader_under_sanitizers(tmp_path, sanitizer):
    """(a) 3 producers hand 200 numbered items through the ticket hand-over into a queue of capacity 2, 3 consumers take their places:
    the offsets are the prefix sums in batch order and every item is seen once; (b) the same with the turn of a non-seekable output:
    written in batch order; (c) fail() while producers and consumers block: every thread returns (5 s at most); (d) ChunkReader with
    a read function that returns 1 - 7 bytes at a time gives the pieces of the fread one, for piece sizes 64 and 4096.  Beyond these:
    the ordered writer's hand-over in normal operation (makers one at a time, host buffers gated, delivery by batch number, end())."""
    src = tmp_path / "stream_parts.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "stream_parts"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "tksm_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe), str(tmp_path / "in.mdf")], capture_output=True, text=True, timeout=5)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
