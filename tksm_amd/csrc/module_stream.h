// module_stream.h -- the host-side plumbing of a streaming module, free of HIP and of the C-ABI so that a stand-alone program can
// compile it (tests/test_stream_parts.py runs it under the thread and address sanitizers): the bounded queue between the stages, the
// ticket hand-over that keeps a group's producers in order, and the order in which finished batches reach the outputs.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <vector>

namespace tkmod {

// bounded; close() ends it: push() then refuses (false, the value stays the caller's), pop() hands out what is queued and then false
template <class T> struct BoundedQueue {
    explicit BoundedQueue(size_t cap) : cap(cap) {}
    bool push(T&& v) {
        std::unique_lock<std::mutex> l(m);
        cv_put.wait(l, [&] { return q.size() < cap || closed; });
        if (closed) return false;
        q.push_back(std::move(v));
        cv_get.notify_one();
        return true;
    }
    bool pop(T& v) {
        std::unique_lock<std::mutex> l(m);
        cv_get.wait(l, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        v = std::move(q.front()); q.pop_front();
        cv_put.notify_one();
        return true;
    }
    void close() { std::lock_guard<std::mutex> l(m); closed = true; cv_get.notify_all(); cv_put.notify_all(); }
private:
    std::mutex m; std::condition_variable cv_put, cv_get; std::deque<T> q; size_t cap; bool closed = false;
};

// Several producers hand their items over in the order in which they took their inputs: take() draws a ticket together with the input
// (one producer at a time), hand() waits for that ticket's turn, runs `h` (push, or free) and lets the next ticket go.  (A worker that
// ran a later batch first would wait for the earlier one's place in the output while that one waits for a worker.)
// `one_at_a_time`: the next producer takes only once the last ticket is handed over (a producer whose take() MAKES the item: no second
// item is made while the first waits for room); take() and hand() of a ticket are then the same thread's.
struct Handover {
    explicit Handover(bool one_at_a_time = false) : one_at_a_time(one_at_a_time) {}
    template <class Take> bool take(uint64_t& ticket, Take&& t) {       // false: `t` had nothing to take, no ticket drawn
        std::unique_lock<std::mutex> l(take_m);
        if (!t()) return false;
        ticket = taken++;
        if (one_at_a_time) l.release();                                 // (unlocked by hand())
        return true;
    }
    template <class Hand> void hand(uint64_t ticket, Hand&& h) {
        {
            std::unique_lock<std::mutex> l(m);
            cv.wait(l, [&] { return handed == ticket; });
            h();
            handed++;
        }
        cv.notify_all();
        if (one_at_a_time) take_m.unlock();
    }
private:
    const bool one_at_a_time;
    std::mutex take_m; uint64_t taken = 0;
    std::mutex m; std::condition_variable cv; uint64_t handed = 0;
};

// a batch whose records wait in its worker's host buffers for the one ordered writer
struct Finished { int worker = -1; uint64_t bytes[2] = {0, 0}; uint64_t n_reads = 0; };

// The order of the batches in (up to) two outputs.  A regular file: batch `seq` takes its place once every earlier batch has announced
// its size.  Anything else is written in batch order: by whoever holds the turn, or by one writer that is handed the finished batches.
// Every wait ends at fail(), and then reports failure.
struct BatchOrder {
    BatchOrder(size_t n_workers, int counted_output) : counted(counted_output), host_busy(n_workers, 0) {}
    bool failed() const { return failed_.load(); }
    void fail() { { std::lock_guard<std::mutex> l(m); failed_ = true; } cv.notify_all(); }    // (under m: no waiter is between its check and its wait)

    // take place k for batch seq: `off` is where its `bytes` go; its reads are counted once, at output `counted_output`
    bool take_place(int k, uint64_t seq, uint64_t bytes, uint64_t n_reads, uint64_t& off) {
        {
            std::unique_lock<std::mutex> l(m);
            cv.wait(l, [&] { return next_place[k] == seq || failed_; });
            if (failed_) return false;
            off = place[k]; place[k] += bytes; next_place[k]++;
            if (k == counted) reads_ += n_reads;
        }
        cv.notify_all();
        return true;
    }
    // my turn to write into a non-seekable output: every batch before `seq` has been written; turn_done() passes the turn on
    bool wait_turn(int k, uint64_t seq) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return written_upto[k] == seq || failed_; });
        return !failed_;
    }
    void turn_done(int k, bool ok) { { std::lock_guard<std::mutex> l(m); if (ok) written_upto[k]++; } cv.notify_all(); }

    // the ordered writer's side.  A worker: wait_host_free() before it fills its host buffers again, finished() once they hold a batch.
    // The writer: next_finished(seq = 0, 1, 2, ...) until false (failed, or all of end()'s batches written), written() after each.
    bool wait_host_free(int worker) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !host_busy[(size_t)worker] || failed_; });
        return !failed_;
    }
    void finished(uint64_t seq, const Finished& f) { { std::lock_guard<std::mutex> l(m); host_busy[(size_t)f.worker] = 1; done[seq] = f; } cv.notify_all(); }
    bool next_finished(uint64_t seq, Finished& f) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return done.count(seq) || failed_ || (ended && seq >= n_batches); });
        if (failed_ || !done.count(seq)) return false;
        f = done[seq]; done.erase(seq);
        return true;
    }
    void written(const Finished& f, bool ok) {
        {
            std::lock_guard<std::mutex> l(m);
            host_busy[(size_t)f.worker] = 0;
            if (ok) { reads_ += f.n_reads; place[0] += f.bytes[0]; place[1] += f.bytes[1]; }
        }
        cv.notify_all();
    }
    void end(uint64_t batches) { { std::lock_guard<std::mutex> l(m); n_batches = batches; ended = true; } cv.notify_all(); }

    uint64_t bytes(int k) { std::lock_guard<std::mutex> l(m); return place[k]; }     // bytes placed / written so far
    uint64_t reads() { std::lock_guard<std::mutex> l(m); return reads_; }
private:
    std::mutex m; std::condition_variable cv; std::atomic<bool> failed_{false};
    const int counted;
    uint64_t next_place[2] = {0, 0}, place[2] = {0, 0}, written_upto[2] = {0, 0}, reads_ = 0;
    std::vector<char> host_busy; std::map<uint64_t, Finished> done;
    uint64_t n_batches = 0; bool ended = false;
};

}  // namespace tkmod
