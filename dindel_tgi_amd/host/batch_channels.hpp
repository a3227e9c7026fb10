// batch_channels.hpp — the hand-overs between the stages of the window loop (dindel_gpu.cpp), header-only, standard library only.
// The pipeline's liveness rests on these three classes; tests/channels_check.cpp exercises them on their own.
// T is the item handed over (the driver: std::unique_ptr<Batch>); push() moves from its argument only when it returns true.
#ifndef DINDEL_BATCH_CHANNELS_HPP
#define DINDEL_BATCH_CHANNELS_HPP
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace dindel {

// hand-over between two pipeline stages: at most `cap` items wait in it
template <class T> class Channel {
public:
    explicit Channel(size_t cap) : cap_(cap), closed_(false) {}
    bool push(T &b)                      // false: the consumer is gone
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return q_.size() < cap_ || closed_; });
        if (closed_) return false;
        q_.push_back(std::move(b));
        cv_.notify_all();
        return true;
    }
    bool pop(T &b)                       // false: closed and drained
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        b = std::move(q_.front());
        q_.pop_front();
        cv_.notify_all();
        return true;
    }
    void close() { std::lock_guard<std::mutex> lk(m_); closed_ = true; cv_.notify_all(); }
    void abort() { std::lock_guard<std::mutex> lk(m_); closed_ = true; q_.clear(); cv_.notify_all(); }     // drops what waits
private:
    std::mutex m_; std::condition_variable cv_; std::deque<T> q_; size_t cap_; bool closed_;
};

// hand-over that restores file order: items may arrive in any order, leave by sequence number (0, 1, 2, ...); an item `cap` or more
// ahead of the next one to leave waits at the door (the one that is next never does, so the stages cannot lock up).
// close(): pop() still hands out the next item if it is here, and returns false at the first gap; abort(): everything is dropped.
template <class T> class OrderedChannel {
public:
    explicit OrderedChannel(long cap) : cap_(cap), next_(0), closed_(false), aborted_(false) {}
    bool push(long seq, T &b)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return seq < next_ + cap_ || aborted_; });
        if (aborted_) return false;
        held_[seq] = std::move(b);
        cv_.notify_all();
        return true;
    }
    bool pop(T &b)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return held_.find(next_) != held_.end() || closed_ || aborted_; });
        return takeNext(b);
    }
    bool tryPop(T &b) { std::lock_guard<std::mutex> lk(m_); return takeNext(b); }     // the next item if it is already here; never waits
    void close() { std::lock_guard<std::mutex> lk(m_); closed_ = true; cv_.notify_all(); }
    void abort() { std::lock_guard<std::mutex> lk(m_); aborted_ = true; held_.clear(); cv_.notify_all(); }
private:
    bool takeNext(T &b)                  // with m_ held
    {
        typename std::map<long, T>::iterator it = held_.find(next_);
        if (aborted_ || it == held_.end()) return false;
        b = std::move(it->second);
        held_.erase(it);
        next_++;
        cv_.notify_all();
        return true;
    }
    std::mutex m_; std::condition_variable cv_; std::map<long, T> held_; long cap_, next_; bool closed_, aborted_;
};

// finished batches on their way back to the reader: what was given back last is taken next (its pages are the warmest); a new B when empty
template <class B> class BatchPool {
public:
    std::unique_ptr<B> take()
    {
        std::lock_guard<std::mutex> lk(m_);
        if (free_.empty()) return std::unique_ptr<B>(new B);
        std::unique_ptr<B> b = std::move(free_.back());
        free_.pop_back();
        return b;
    }
    void give(std::unique_ptr<B> &b) { std::lock_guard<std::mutex> lk(m_); free_.push_back(std::move(b)); }
private:
    std::mutex m_; std::vector<std::unique_ptr<B> > free_;
};

} // namespace dindel
#endif
