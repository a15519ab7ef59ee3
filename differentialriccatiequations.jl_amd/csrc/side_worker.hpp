// One parked host thread for work that is DRIVEN beside a time loop (the side-stream compression of X has host read-backs of its own, so it
// cannot simply be enqueued): jobs are handed over through a condition variable — no thread is spawned per time step.  Nothing of HIP in here.
#pragma once
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>

namespace dre {

class SideWorker {
  public:
    // Owner of the ONE job in flight.  What the job reads must outlive the handle: wait() joins and rethrows what the job threw, the destructor
    // (and reset()) joins and swallows it — declare the handle behind everything the job refers to.  Move-only; a moved-from handle is empty.
    class Job {
      public:
        Job() = default;
        Job(Job&& o) noexcept : w_(std::exchange(o.w_, nullptr)), seq_(o.seq_) {}
        Job& operator=(Job&& o) noexcept { if (this != &o) { reset(); w_ = std::exchange(o.w_, nullptr); seq_ = o.seq_; } return *this; }
        Job(const Job&) = delete;
        Job& operator=(const Job&) = delete;
        ~Job() { reset(); }
        bool pending() const { return w_ != nullptr; }      // still owns an unjoined job
        void wait() { if (w_) std::exchange(w_, nullptr)->join(seq_, true); }
        void reset() noexcept { if (w_) { try { std::exchange(w_, nullptr)->join(seq_, false); } catch (...) {} } }
      private:
        friend class SideWorker;
        Job(SideWorker* w, unsigned long seq) : w_(w), seq_(seq) {}
        SideWorker* w_ = nullptr;
        unsigned long seq_ = 0;
    };

    ~SideWorker() { { std::lock_guard<std::mutex> lk(m_); quit_ = true; } cv_.notify_all(); if (th_.joinable()) th_.join(); }
    // ONE job at a time: a second submission waits for the first instead of replacing it.  The error of a job nobody joined (its handle was
    // overwritten by this submission's) stays for the next wait().
    Job submit(std::function<void()> job) {
        if (!th_.joinable()) th_ = std::thread([this] { run(); });
        unsigned long seq;
        {
            std::unique_lock<std::mutex> lk(m_);
            done_.wait(lk, [this] { return !busy_; });
            job_ = std::move(job); busy_ = true; seq = ++submitted_;
        }
        cv_.notify_all();
        return Job(this, seq);
    }
    bool pending() { std::lock_guard<std::mutex> lk(m_); return busy_; }      // the thread is at work (whoever owns the job)
  private:
    // returns when job `seq` is finished.  rethrow: hands out the kept error; otherwise the error is dropped, unless a later job was
    // submitted since (then it is not this handle's to drop: it stays for that job's wait())
    void join(unsigned long seq, bool rethrow) {
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return finished_ >= seq; });
        if (!err_ || (!rethrow && submitted_ != seq)) return;
        auto e = std::exchange(err_, nullptr);
        if (rethrow) std::rethrow_exception(e);
    }
    void run() {
        for (;;) {
            std::function<void()> job;
            { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [this] { return quit_ || (busy_ && job_); }); if (quit_) return; job = std::move(job_); job_ = nullptr; }
            std::exception_ptr e;
            try { job(); } catch (...) { e = std::current_exception(); }
            { std::lock_guard<std::mutex> lk(m_); busy_ = false; ++finished_; if (e || !err_) err_ = e; }
            done_.notify_all();
        }
    }
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::function<void()> job_;
    std::exception_ptr err_;
    unsigned long submitted_ = 0, finished_ = 0;
    bool busy_ = false, quit_ = false;
};

}  // namespace dre
