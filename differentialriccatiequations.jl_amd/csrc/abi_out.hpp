// One owner for the result handles of a C ABI entry point (api*.hip).  An entry point makes every handle it returns through make(slot); the
// caller's slots are written by commit() alone, all of them together, when nothing can throw any more.  An AbiOut that goes out of scope
// without commit() (an argument check or a solver threw) deletes what it holds and leaves every slot as the entry point left it: untouched in
// the single calls, null in the batched calls, which null their arrays up front and make handles for the live members only.
// Plain host C++ without any HIP type, so that a stand-alone program can test it (tests/test_abi_out_host.py).
#pragma once
#include <memory>
#include <vector>

namespace dre {

template <typename H>
class AbiOut {
public:
    AbiOut() = default;
    AbiOut(const AbiOut&) = delete;
    AbiOut& operator=(const AbiOut&) = delete;
    ~AbiOut() { for (Held& e : held_) delete e.h; }
    // a fresh handle meant for *slot (one result, one of a group, member b of an array: slot = X + b)
    H* make(H** slot) {
        std::unique_ptr<H> h(new H());
        held_.push_back(Held{slot, h.get()});
        return h.release();
    }
    void commit() noexcept {
        for (Held& e : held_) *e.slot = e.h;
        held_.clear();
    }

private:
    struct Held { H** slot; H* h; };
    std::vector<Held> held_;
};

}  // namespace dre
