// Stand-alone check of the pin table (simpleraytracer_amd/csrc/pin_table.h), the host bookkeeping of
// DeviceScene's pinned offsets: lookup, the cap, a pin again, the drop on a resize, the deferred
// release, and the summary state (unknown / regular / other) with its generations. The table makes no HIP call, so this builds and runs anywhere, under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Isimpleraytracer_amd/csrc tools/pin_table_check.cpp -o pin_table_check && ./pin_table_check
// The "facts buffers", summary words and events are heap blocks of this program: a block freed twice,
// leaked or read after its release is what the sanitizers would report.
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
    const std::vector<srt::PinTable::Buffers> gone = t.TakeRetired();
    for (const srt::PinTable::Buffers& b : gone) {
        std::free(b.facts);
        std::free(b.word);  // (null for the pins made without a summary: free(nullptr) does nothing)
        std::free(b.event);
    }
    return gone.size();
}

// A pin with a summary word and an "event" of its own, as the owner makes them.
srt::PinTable::Buffers NewPin(unsigned char fill) {
    srt::PinTable::Buffers b;
    b.facts = NewFacts(fill);
    b.word = std::calloc(1, sizeof(unsigned));
    b.event = std::malloc(1);
    return b;
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

    // The summary. A fresh pin is unknown; the owner sets what it read for the pin's generation.
    const PinTable::Buffers pa = NewPin(1), pb = NewPin(2);
    Expect(t.Insert(&keys[0], pa) && t.Insert(&keys[1], pb), "two pins with summary words");
    Expect(t.FindBuffers(&keys[0]).word == pa.word && t.FindBuffers(&keys[0]).event == pa.event &&
               t.FindBuffers(&keys[2]).facts == nullptr,
           "a pin keeps its word and event");
    Expect(t.summary(&keys[0]) == PinTable::kUnknown && t.summary(&keys[2]) == PinTable::kUnknown,
           "a fresh pin's summary is unknown, and so is an unpinned key's");
    Expect(t.Pending().size() == 2, "both wait for their summaries");
    Expect(!t.SetSummary(&keys[0], 0u, PinTable::kUnknown), "unknown is not a summary to set");
    Expect(!t.SetSummary(&keys[2], 0u, PinTable::kRegular), "nor is there one for an unpinned key");
    Expect(t.SetSummary(&keys[0], t.generation(&keys[0]), PinTable::kRegular) && t.summary(&keys[0]) == PinTable::kRegular,
           "the summary read for the pin's generation stands");
    Expect(t.SetSummary(&keys[1], 0u, PinTable::kOther) && t.summary(&keys[1]) == PinTable::kOther, "regular or not");
    Expect(!t.SetSummary(&keys[0], 0u, PinTable::kOther) && t.summary(&keys[0]) == PinTable::kRegular,
           "a known summary is not overwritten");
    Expect(t.Pending().empty(), "nothing waits any more");
    // A re-pin: unknown before the facts launch is queued, and the old generation's word is refused.
    const unsigned g0 = t.generation(&keys[0]);
    const unsigned g1 = t.MarkPending(&keys[0]);
    Expect(g1 != g0 && g1 != 0u && t.generation(&keys[0]) == g1, "a re-pin starts a new generation");
    Expect(t.summary(&keys[0]) == PinTable::kUnknown && t.Pending().size() == 1, "whose summary is unknown");
    Expect(t.Find(&keys[0]) == pa.facts, "in the same buffer");
    Expect(!t.SetSummary(&keys[0], g0, PinTable::kRegular) && t.summary(&keys[0]) == PinTable::kUnknown,
           "a stale summary (the old generation's) is refused");
    const unsigned g2 = t.MarkPending(&keys[0]);
    Expect(g2 != g1 && !t.SetSummary(&keys[0], g1, PinTable::kRegular), "and so is the one of a re-pin overtaken by another");
    Expect(t.SetSummary(&keys[0], g2, PinTable::kOther) && t.summary(&keys[0]) == PinTable::kOther,
           "the newest generation's is taken");
    Expect(t.MarkPending(&keys[2]) == 0u && t.summary(&keys[1]) == PinTable::kOther, "a re-pin of nothing changes nothing");
    // Remove and clear retire the word and the event with the buffer, and forget the state.
    Expect(t.Remove(&keys[0]) && t.summary(&keys[0]) == PinTable::kUnknown && t.generation(&keys[0]) == 0u,
           "an unpin forgets the summary");
    Expect(t.retired() == 1 && *static_cast<unsigned*>(pa.word) == 0u, "its word lives until the release");
    const PinTable::Buffers pa2 = NewPin(3);
    Expect(t.Insert(&keys[0], pa2) && t.summary(&keys[0]) == PinTable::kUnknown && t.FindBuffers(&keys[0]).word == pa2.word,
           "the address pinned anew starts unknown, with its own word");
    t.Clear();
    Expect(t.summary(&keys[1]) == PinTable::kUnknown && t.Pending().empty() && t.retired() == 3, "a resize drops the summaries too");
    Expect(Release(t) == 3, "and every facts buffer, word and event is released once");

    std::printf(failures == 0 ? "pin_table_check: ok\n" : "pin_table_check: %d FAILED\n", failures);
    return failures == 0 ? 0 : 1;
}
