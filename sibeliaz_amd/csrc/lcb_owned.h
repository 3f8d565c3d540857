// lcb_owned.h — one owner for what a device holds (device.hip): every allocation, stream and event is registered where it is
// made and released from the registration, so that destroying a device (or giving up a half-made one) names nothing.
// Plain C++ without any HIP call: the owner is told how to release a resource of each kind (tests/emu/owned_emu.cpp drives it
// with stubs in place of the hip* functions).
#ifndef LCB_OWNED_H
#define LCB_OWNED_H

#include <vector>

enum LcbOwnedKind { LCB_OWN_DEVICE, LCB_OWN_PINNED, LCB_OWN_STREAM, LCB_OWN_EVENT };

class LcbOwner {
public:
    typedef int (*Release)(LcbOwnedKind kind, void* p);      // 0 = released (the hip* status in device.hip)
    explicit LcbOwner(Release r) : release_(r) {}
    LcbOwner(const LcbOwner&) = delete;
    LcbOwner& operator=(const LcbOwner&) = delete;
    ~LcbOwner() { releaseAll(); }

    // Makes and registers a resource: alloc() returns it or throws. Its place in the list exists before the resource does, so nothing
    // can fail between making it and owning it.
    template <class Alloc>
    void* make(LcbOwnedKind kind, Alloc alloc)
    {
        items_.push_back(Item{kind, nullptr});
        try { items_.back().p = alloc(); } catch (...) { items_.pop_back(); throw; }
        return items_.back().p;
    }

    // Releases one resource now (a buffer that is about to be made again in another size) and forgets it. Returns the status of the release.
    int drop(void* p)
    {
        if (!p) return 0;
        for (size_t i = items_.size(); i-- > 0;)
            if (items_[i].p == p) {
                const LcbOwnedKind kind = items_[i].kind;
                items_.erase(items_.begin() + (long)i);
                return release_(kind, p);
            }
        return -1;      // not ours
    }

    // Everything that is still registered, the youngest first (streams and events are made before what runs on them).
    void releaseAll()
    {
        while (!items_.empty()) {
            const Item it = items_.back();
            items_.pop_back();
            if (it.p) (void)release_(it.kind, it.p);
        }
    }

    size_t size() const { return items_.size(); }

private:
    struct Item { LcbOwnedKind kind; void* p; };
    std::vector<Item> items_;
    Release release_;
};

#endif
