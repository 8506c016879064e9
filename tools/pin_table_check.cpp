// Stand-alone check of the pin table (simpleraytracer_amd/csrc/pin_table.h), the host bookkeeping of
// DeviceScene's pinned offsets: lookup, the cap, a pin again, the drop on a resize and the deferred
// release. The table makes no HIP call, so this builds and runs anywhere, under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Isimpleraytracer_amd/csrc tools/pin_table_check.cpp -o pin_table_check && ./pin_table_check
// The "facts buffers" are heap blocks of this program: a block freed twice, leaked or read after its
// release is what the sanitizers would report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pin_table.h"

namespace {

int failures = 0;

void Expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

constexpr std::size_t kFactsBytes = 40 * 16;  // a 4 x 10 tile grid

void* NewFacts(unsigned char fill) {
    void* p = std::malloc(kFactsBytes);
    std::memset(p, fill, kFactsBytes);
    return p;
}

// The owner's release: what TakeRetired hands over is freed exactly once.
std::size_t Release(srt::PinTable& t) {
    const std::vector<void*> gone = t.TakeRetired();
    for (void* p : gone) {
        std::free(p);
    }
    return gone.size();
}

}  // namespace

int main() {
    using srt::PinTable;
    static_assert(PinTable::kMaxPins >= 64, "the rotating-inputs leg pins 16 buffers per queue scene; the cap is 64");
    std::vector<float> keys(PinTable::kMaxPins + 1);  // (addresses only: never read)

    PinTable t;
    Expect(t.empty() && t.size() == 0 && !t.full() && t.retired() == 0, "a new table is empty");
    Expect(t.Find(&keys[0]) == nullptr && t.Find(nullptr) == nullptr, "nothing is pinned in it");
    Expect(!t.Remove(&keys[0]) && t.retired() == 0, "removing what is not pinned retires nothing");

    // Lookup.
    void* a = NewFacts(1);
    void* b = NewFacts(2);
    Expect(t.Insert(&keys[0], a) && t.Insert(&keys[1], b), "two pins");
    Expect(t.Find(&keys[0]) == a && t.Find(&keys[1]) == b && t.Find(&keys[2]) == nullptr, "each key finds its own buffer");
    Expect(t.size() == 2, "size counts the pins");

    // A pin again: the owner rewrites the buffer Find gives; a second insert is refused, nothing changes.
    void* spare = NewFacts(3);
    Expect(!t.Insert(&keys[0], spare) && t.Find(&keys[0]) == a && t.size() == 2, "a pinned key is not inserted twice");
    Expect(!t.Insert(nullptr, spare) && !t.Insert(&keys[2], nullptr) && t.size() == 2, "null key or buffer is refused");
    std::free(spare);
    std::memset(t.Find(&keys[0]), 9, kFactsBytes);  // (new contents into the standing buffer)
    Expect(static_cast<unsigned char*>(a)[kFactsBytes - 1] == 9, "a pin again writes the same buffer");

    // Deferred release: a removed pin is no longer found, its buffer lives until the owner takes it.
    Expect(t.Remove(&keys[0]) && t.Find(&keys[0]) == nullptr && t.size() == 1, "remove forgets the pin");
    Expect(t.retired() == 1, "its buffer waits for the release");
    Expect(static_cast<unsigned char*>(a)[0] == 9, "and is still readable (queued work may read it)");
    Expect(!t.Remove(&keys[0]) && t.retired() == 1, "a second remove does nothing");
    // The same address pinned anew gets the new buffer, never the retired one.
    void* a2 = NewFacts(4);
    Expect(t.Insert(&keys[0], a2) && t.Find(&keys[0]) == a2, "an address pinned again after an unpin gets a new buffer");
    Expect(Release(t) == 1 && t.retired() == 0, "the release hands each retired buffer over once");
    Expect(Release(t) == 0, "and then none");

    // The cap: kMaxPins pins, one more is refused and evicts nothing.
    for (std::size_t i = 2; i < PinTable::kMaxPins; ++i) {
        Expect(t.Insert(&keys[i], NewFacts(static_cast<unsigned char>(i))), "pins up to the cap");
    }
    Expect(t.full() && t.size() == PinTable::kMaxPins, "the table is full at the cap");
    void* extra = NewFacts(7);
    Expect(!t.Insert(&keys[PinTable::kMaxPins], extra), "one more pin is refused");
    std::free(extra);
    Expect(t.size() == PinTable::kMaxPins && t.retired() == 0, "and nothing was evicted for it");
    bool all = true;
    for (std::size_t i = 0; i < PinTable::kMaxPins; ++i) {
        all = all && t.Find(&keys[i]) != nullptr;
    }
    Expect(all, "every pin still stands");
    Expect(t.Find(&keys[PinTable::kMaxPins - 1]) != nullptr &&
               static_cast<unsigned char*>(t.Find(&keys[PinTable::kMaxPins - 1]))[0] == PinTable::kMaxPins - 1,
           "the last pin finds its own buffer");
    // A slot freed by an unpin can be taken again.
    Expect(t.Remove(&keys[5]) && !t.full(), "an unpin makes room");
    Expect(t.Insert(&keys[PinTable::kMaxPins], NewFacts(8)) && t.full(), "for another pin");

    // The drop on a resize: every pin goes, every buffer waits for the release.
    const std::size_t standing = t.size(), waiting = t.retired();
    t.Clear();
    Expect(t.empty() && t.Find(&keys[1]) == nullptr, "a resize drops every pin");
    Expect(t.retired() == standing + waiting, "and retires every buffer");
    Expect(Release(t) == standing + waiting, "which the owner then frees");
    t.Clear();
    Expect(t.empty() && t.retired() == 0, "clearing an empty table does nothing");
    void* again = NewFacts(5);
    Expect(t.Insert(&keys[1], again) && t.Find(&keys[1]) == again, "pinning again after the drop works");
    t.Clear();
    Release(t);  // (the owner's teardown)

    std::printf(failures == 0 ? "pin_table_check: ok\n" : "pin_table_check: %d FAILED\n", failures);
    return failures == 0 ? 0 : 1;
}
