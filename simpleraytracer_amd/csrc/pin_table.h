// The pinned sample-offset buffers of a DeviceScene (renderer.h "Pinned offsets"): which caller
// buffers have their tile facts stored, in which facts buffer, and what is known about them. Host
// bookkeeping only: no HIP call is made here, the owner allocates and frees
// (tools/pin_table_check.cpp exercises it alone).
//
// A pin maps the caller's offsets pointer to a facts buffer the owner allocated. Removing a pin does
// not free its buffer: queued work may still read it. The buffer moves to the retired list, and the
// owner frees what TakeRetired() hands over once the work that could read it has finished.
//
// A pin's summary says whether every tile of the buffer is regular, usable and in range (a launch
// of such pins alone may run the trace without the position table). The owner computes it on the
// device behind the facts launch, into the pin's `word`, and signals it with the pin's `event`; both
// are the owner's, opaque here, and retire with the facts buffer. The table only keeps the state:
//   unknown: the facts launch (or a re-pin's) is queued and its summary has not been read yet;
//   regular / other: read from the word after the event of that very launch completed.
// A re-pin rewrites the facts, so MarkPending() puts the state back to unknown *before* the owner
// queues the new facts launch, and bumps the pin's generation: a summary is taken only for the
// generation it was computed for (SetSummary), so a stale "regular" cannot come back.
#pragma once

#include <cstddef>
#include <vector>

namespace srt {

class PinTable {
public:
    // Pins per table. One more is refused, never an eviction: a caller that pinned a buffer relies
    // on it staying pinned.
    static constexpr std::size_t kMaxPins = 64;

    enum Summary { kUnknown = 0, kRegular = 1, kOther = 2 };

    // What the owner allocated for one pin, and gets back from TakeRetired().
    struct Buffers {
        void* facts = nullptr;
        void* word = nullptr;   // the summary word, readable by the host
        void* event = nullptr;  // completes when the word is written
    };

    std::size_t size() const { return m_pins.size(); }
    bool empty() const { return m_pins.empty(); }
    bool full() const { return m_pins.size() >= kMaxPins; }

    // The facts buffer of `key`, or null: not pinned.
    void* Find(const void* key) const {
        const Pin* p = Get(key);
        return p != nullptr ? p->buf.facts : nullptr;
    }
    // All of a pin's buffers (facts null: not pinned).
    Buffers FindBuffers(const void* key) const {
        const Pin* p = Get(key);
        return p != nullptr ? p->buf : Buffers{};
    }

    // A new pin, its summary unknown. False, and nothing changed: the key is null or pinned already
    // (a re-pin rewrites the buffer Find gives), `facts` is null, or the table is full.
    bool Insert(const void* key, const Buffers& buf) {
        if (key == nullptr || buf.facts == nullptr || full() || Find(key) != nullptr) {
            return false;
        }
        m_pins.push_back(Pin{key, buf, kUnknown, 0u});
        return true;
    }
    bool Insert(const void* key, void* facts) { return Insert(key, Buffers{facts, nullptr, nullptr}); }

    // The summary of `key` (kUnknown also for a key that is not pinned).
    Summary summary(const void* key) const {
        const Pin* p = Get(key);
        return p != nullptr ? p->summary : kUnknown;
    }
    // The generation of `key`'s facts: what MarkPending last returned (0: a fresh pin, or not pinned).
    unsigned generation(const void* key) const {
        const Pin* p = Get(key);
        return p != nullptr ? p->generation : 0u;
    }
    // A re-pin is about to rewrite `key`'s facts: the summary is unknown from now on. Returns the new
    // generation (0: not pinned, nothing changed). Call before the facts launch is queued.
    unsigned MarkPending(const void* key) {
        Pin* p = Get(key);
        if (p == nullptr) {
            return 0u;
        }
        p->summary = kUnknown;
        p->generation = p->generation + 1u == 0u ? 1u : p->generation + 1u;
        return p->generation;
    }
    // The summary the owner read for `generation`. False, and nothing changed: not pinned, `s` is
    // kUnknown, the summary is known already, or the facts are of another generation by now.
    bool SetSummary(const void* key, unsigned generation, Summary s) {
        Pin* p = Get(key);
        if (p == nullptr || s == kUnknown || p->summary != kUnknown || p->generation != generation) {
            return false;
        }
        p->summary = s;
        return true;
    }
    // The keys whose summary is unknown (the owner polls or waits for their events).
    std::vector<const void*> Pending() const {
        std::vector<const void*> out;
        for (const Pin& p : m_pins) {
            if (p.summary == kUnknown) {
                out.push_back(p.key);
            }
        }
        return out;
    }

    // Forgets `key`; its buffers are retired. False: it was not pinned.
    bool Remove(const void* key) {
        for (std::size_t i = 0; i < m_pins.size(); ++i) {
            if (m_pins[i].key == key) {
                m_retired.push_back(m_pins[i].buf);
                m_pins.erase(m_pins.begin() + static_cast<std::ptrdiff_t>(i));
                return true;
            }
        }
        return false;
    }

    // Forgets every pin (the frame size changed: the facts are of another tile grid).
    void Clear() {
        for (const Pin& p : m_pins) {
            m_retired.push_back(p.buf);
        }
        m_pins.clear();
    }

    // Buffers waiting for their release.
    std::size_t retired() const { return m_retired.size(); }
    // Hands the retired buffers to the owner, which frees them after the work that may read them.
    std::vector<Buffers> TakeRetired() {
        std::vector<Buffers> out;
        out.swap(m_retired);
        return out;
    }

private:
    struct Pin {
        const void* key;
        Buffers buf;
        Summary summary;
        unsigned generation;
    };
    const Pin* Get(const void* key) const {
        for (const Pin& p : m_pins) {
            if (p.key == key) {
                return &p;
            }
        }
        return nullptr;
    }
    Pin* Get(const void* key) { return const_cast<Pin*>(static_cast<const PinTable*>(this)->Get(key)); }

    std::vector<Pin> m_pins;
    std::vector<Buffers> m_retired;
};

}  // namespace srt
