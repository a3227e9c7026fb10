// channels_check — the window loop's hand-overs (host/batch_channels.hpp: Channel, OrderedChannel, BatchPool) on their own: a few threads,
// small caps, no GPU, standard library only.  tests/test_channels_cpu.py builds and runs it; it also builds with -fsanitize=thread.
// Blocking is checked with a flag the blocked thread sets after its call returns: read before and after the releasing action.  The program
// never hangs: every check runs against a deadline kept by a watchdog thread, which names the check and leaves with status 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include "../dindel_tgi_amd/host/batch_channels.hpp"

using namespace dindel;
typedef std::unique_ptr<int> Item;

namespace {
const int kDeadlineMs = 5000, kSettleMs = 50;
std::atomic<const char *> checkName("start");
std::atomic<long long> deadline(0);
std::atomic<bool> finished(false);
int failures = 0;

long long nowMs() { return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void snooze(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }
void begin(const char *name) { checkName = name; deadline = nowMs() + kDeadlineMs; }
void watchdog()
{
    while (!finished) {
        if (nowMs() > deadline) { printf("TIMED OUT: %s\n", checkName.load()); fflush(stdout); std::_Exit(1); }
        snooze(5);
    }
}
void expect(bool ok, const char *what)
{
    if (!ok) { printf("FAILED: %s: %s\n", checkName.load(), what); failures++; }
}
Item item(int v) { return Item(new int(v)); }

// a thread whose end the main thread can see: `done` is set after the body has returned
class Worker {
public:
    template <class F> explicit Worker(F body) : done(false), t([this, body]() { body(); done = true; }) {}
    void join() { while (!done) snooze(1); t.join(); }         // (the watchdog ends the program if this never happens)
    std::atomic<bool> done;
private:
    std::thread t;
};

void channelChecks()
{
    begin("Channel: three producers, every item once and in each producer's push order");
    {
        Channel<Item> ch(2);
        const int per = 200;
        std::vector<std::unique_ptr<Worker> > producers;
        for (int p = 0; p < 3; p++) producers.push_back(std::unique_ptr<Worker>(new Worker([&ch, p]() { for (int k = 0; k < per; k++) { Item x = item(p * 1000 + k); ch.push(x); } })));
        Worker closer([&]() { for (size_t p = 0; p < producers.size(); p++) producers[p]->join(); ch.close(); });
        int nextOf[3] = {0, 0, 0}, total = 0;
        Item x;
        while (ch.pop(x)) { const int p = *x / 1000, k = *x % 1000; expect(p >= 0 && p < 3 && k == nextOf[p], "out of order"); if (p >= 0 && p < 3) nextOf[p] = k + 1; total++; }
        closer.join();
        expect(total == 3 * per, "item count");
        expect(!ch.pop(x), "pop after close and drain");
    }
    begin("Channel: push blocks at the cap and is released by a pop");
    {
        Channel<Item> ch(2);
        Item a = item(1), b = item(2), out;
        expect(ch.push(a) && ch.push(b) && !a && !b, "pushes below the cap");
        std::atomic<bool> ok(false);
        Worker third([&]() { Item c = item(3); ok = ch.push(c); });
        snooze(kSettleMs);
        expect(!third.done, "third push returned although two items wait");
        expect(ch.pop(out) && *out == 1, "first item");
        third.join();
        expect(ok, "released push reports success");
        expect(ch.pop(out) && *out == 2 && ch.pop(out) && *out == 3, "push order");
    }
    begin("Channel: close drains, then pop and push return false");
    {
        Channel<Item> ch(4);
        Item a = item(1), b = item(2), c = item(3), out;
        ch.push(a); ch.push(b);
        ch.close();
        expect(!ch.push(c) && c && *c == 3, "push after close keeps its item");
        expect(ch.pop(out) && *out == 1 && ch.pop(out) && *out == 2, "drained in order");
        expect(!ch.pop(out), "pop when closed and drained");
    }
    begin("Channel: abort drops what waits and releases a blocked push and a blocked pop");
    {
        Channel<Item> ch(1), empty(1);
        Item a = item(1), out;
        ch.push(a);
        std::atomic<bool> pushed(true), popped(true);
        Worker pusher([&]() { Item b = item(2); pushed = ch.push(b); });
        Worker popper([&]() { Item got; popped = empty.pop(got); });
        snooze(kSettleMs);
        expect(!pusher.done && !popper.done, "blocked before the abort");
        ch.abort(); empty.abort();
        pusher.join(); popper.join();
        expect(!pushed && !popped, "released calls return false");
        expect(!ch.pop(out), "pop after abort (the waiting item is dropped)");
        expect(!ch.push(a), "push after abort");
    }
}

void orderedChecks()
{
    begin("OrderedChannel: four pushers, arrival order scrambled, leave in sequence order");
    {
        OrderedChannel<Item> ch(3);
        const int total = 400;
        std::vector<std::unique_ptr<Worker> > pushers;      // pusher p holds p, p + 4, ...: like a stage's workers, each one's own numbers ascend
        for (int p = 0; p < 4; p++) pushers.push_back(std::unique_ptr<Worker>(new Worker([&ch, p]() {
            for (int s = p; s < total; s += 4) { if ((s * 7 + p) % 5 == 0) std::this_thread::yield(); Item x = item(s); ch.push(s, x); }
        })));
        Item x;
        for (int s = 0; s < total; s++) expect(ch.pop(x) && *x == s, "sequence order");
        for (size_t p = 0; p < pushers.size(); p++) pushers[p]->join();
        expect(!ch.tryPop(x), "nothing left");
    }
    begin("OrderedChannel: one pusher, a fixed permutation inside the cap");
    {
        OrderedChannel<Item> ch(8);
        const int order[8] = {5, 2, 7, 0, 3, 6, 1, 4};
        Item x;
        for (int k = 0; k < 8; k++) { x = item(order[k]); expect(ch.push(order[k], x), "push inside the cap"); }
        for (int s = 0; s < 8; s++) expect(ch.pop(x) && *x == s, "sequence order");
    }
    begin("OrderedChannel: a pusher `cap` ahead waits while the next item is missing; the next one never waits");
    {
        OrderedChannel<Item> ch(2);
        Item one = item(1), out;
        expect(ch.push(1, one), "an item less than cap ahead goes in");
        std::vector<int> got;
        Worker consumer([&]() { Item x; for (int k = 0; k < 3 && ch.pop(x); k++) got.push_back(*x); });
        std::atomic<bool> ok(false);
        Worker ahead([&]() { Item two = item(2); ok = ch.push(2, two); });
        snooze(kSettleMs);
        expect(!ahead.done, "push of number 2 returned while number 0 is missing (cap 2)");
        expect(!consumer.done && got.empty(), "pop handed out something before number 0 came");
        Item zero = item(0);
        expect(ch.push(0, zero), "the next item goes in at once");
        ahead.join(); consumer.join();
        expect(ok, "released push reports success");
        expect(got.size() == 3 && got[0] == 0 && got[1] == 1 && got[2] == 2, "sequence order");
    }
    begin("OrderedChannel: tryPop never waits");
    {
        OrderedChannel<Item> ch(4);
        Item x, one = item(1), zero = item(0);
        expect(!ch.tryPop(x), "empty");
        ch.push(1, one);
        expect(!ch.tryPop(x), "only number 1 is here");
        ch.push(0, zero);
        expect(ch.tryPop(x) && *x == 0 && ch.tryPop(x) && *x == 1 && !ch.tryPop(x), "0, 1, then nothing");
    }
    begin("OrderedChannel: close hands out up to the first gap; a waiting pop is released");
    {
        OrderedChannel<Item> ch(4), empty(4);
        Item x, zero = item(0), two = item(2);
        ch.push(0, zero); ch.push(2, two);
        std::atomic<bool> popped(true);
        Worker popper([&]() { Item got; popped = empty.pop(got); });
        snooze(kSettleMs);
        expect(!popper.done, "pop on an empty channel waits");
        ch.close(); empty.close();
        popper.join();
        expect(!popped, "released pop returns false");
        expect(ch.pop(x) && *x == 0, "number 0 still leaves");
        expect(!ch.pop(x) && !ch.tryPop(x), "number 1 never came: false");
    }
    begin("OrderedChannel: abort releases a pusher waiting at the door");
    {
        OrderedChannel<Item> ch(1);
        std::atomic<bool> ok(true);
        Worker ahead([&]() { Item one = item(1); ok = ch.push(1, one); });
        snooze(kSettleMs);
        expect(!ahead.done, "number 1 waits at the door (cap 1)");
        ch.abort();
        ahead.join();
        Item x, zero = item(0);
        expect(!ok, "released push returns false");
        expect(!ch.push(0, zero) && !ch.pop(x) && !ch.tryPop(x), "everything returns false after abort");
    }
}

void poolChecks()
{
    begin("BatchPool: what is given back is what is taken next");
    BatchPool<int> pool;
    std::unique_ptr<int> a = pool.take(), b = pool.take();
    expect(a && b && a.get() != b.get(), "an empty pool makes new items");
    int *pa = a.get(), *pb = b.get();
    pool.give(a);
    expect(!a, "give takes the item");
    a = pool.take();
    expect(a.get() == pa, "the one given back");
    pool.give(a); pool.give(b);
    b = pool.take(); a = pool.take();
    expect(b.get() == pb && a.get() == pa, "the last one given back first");
    std::unique_ptr<int> c = pool.take();
    expect(c && c.get() != pa && c.get() != pb, "empty again: a new item");
}
}

int main()
{
    begin("start");
    std::thread dog(watchdog);
    channelChecks();
    orderedChecks();
    poolChecks();
    finished = true;
    dog.join();
    if (failures) printf("channels_check: %d FAILED\n", failures); else printf("channels_check: ok\n");
    return failures ? 1 : 0;
}
