// The pinned sample-offset buffers of a DeviceScene (renderer.h "Pinned offsets"): which caller
// buffers have their tile facts stored, and in which facts buffer. Host bookkeeping only: no HIP
// call is made here, the owner allocates and frees (tools/pin_table_check.cpp exercises it alone).
//
// A pin maps the caller's offsets pointer to a facts buffer the owner allocated. Removing a pin does
// not free its buffer: queued work may still read it. The buffer moves to the retired list, and the
// owner frees what TakeRetired() hands over once the work that could read it has finished.
#pragma once

#include <cstddef>
#include <vector>

namespace srt {

class PinTable {
public:
    // Pins per table. One more is refused, never an eviction: a caller that pinned a buffer relies
    // on it staying pinned.
    static constexpr std::size_t kMaxPins = 64;

    std::size_t size() const { return m_pins.size(); }
    bool empty() const { return m_pins.empty(); }
    bool full() const { return m_pins.size() >= kMaxPins; }

    // The facts buffer of `key`, or null: not pinned.
    void* Find(const void* key) const {
        for (const Pin& p : m_pins) {
            if (p.key == key) {
                return p.facts;
            }
        }
        return nullptr;
    }

    // A new pin. False, and nothing changed: the key is null or pinned already (a re-pin rewrites
    // the buffer Find gives), `facts` is null, or the table is full.
    bool Insert(const void* key, void* facts) {
        if (key == nullptr || facts == nullptr || full() || Find(key) != nullptr) {
            return false;
        }
        m_pins.push_back(Pin{key, facts});
        return true;
    }

    // Forgets `key`; its buffer is retired. False: it was not pinned.
    bool Remove(const void* key) {
        for (std::size_t i = 0; i < m_pins.size(); ++i) {
            if (m_pins[i].key == key) {
                m_retired.push_back(m_pins[i].facts);
                m_pins.erase(m_pins.begin() + static_cast<std::ptrdiff_t>(i));
                return true;
            }
        }
        return false;
    }

    // Forgets every pin (the frame size changed: the facts are of another tile grid).
    void Clear() {
        for (const Pin& p : m_pins) {
            m_retired.push_back(p.facts);
        }
        m_pins.clear();
    }

    // Buffers waiting for their release.
    std::size_t retired() const { return m_retired.size(); }
    // Hands the retired buffers to the owner, which frees them after the work that may read them.
    std::vector<void*> TakeRetired() {
        std::vector<void*> out;
        out.swap(m_retired);
        return out;
    }

private:
    struct Pin {
        const void* key;
        void* facts;
    };
    std::vector<Pin> m_pins;
    std::vector<void*> m_retired;
};

}  // namespace srt
