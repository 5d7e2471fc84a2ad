// Which LoRA adapter slots are loaded, under which uid, and how many queued or running requests name each (no counterpart in the
// reference, whose engine serves one set of weights).  The backend writes it (HipResourceManager::LoadAdapter / UnloadAdapter), the
// generator reads it: a request takes a reference on its slot when it is queued and drops it when it leaves, so that a slot is never
// unloaded under a request, and the uid seeds the request's prefix-cache hash chain -- K/V computed under an adapter are not the base
// model's, and a reloaded slot gets a new uid, so pages of the adapter it held before never hit and age out by LRU.
#pragma once
#include <stdint.h>

#include <mutex>

namespace ppl { namespace llm {

class AdapterRegistry final {
public:
    static constexpr int kMaxSlots = 64;   // PPLHIP_LORA_MAX_SLOTS

    // a request names `slot`: its uid (never 0) and a reference on the slot, or false when nothing is loaded there
    bool Acquire(int slot, uint64_t* uid) {
        std::lock_guard<std::mutex> g(mu_);
        if (slot < 0 || slot >= kMaxSlots || uid_[slot] == 0) return false;
        ++refs_[slot];
        *uid = uid_[slot];
        return true;
    }
    void Release(int slot) {
        std::lock_guard<std::mutex> g(mu_);
        if (slot >= 0 && slot < kMaxSlots && refs_[slot] > 0) --refs_[slot];
    }
    bool IsLoaded(int slot) {
        std::lock_guard<std::mutex> g(mu_);
        return slot >= 0 && slot < kMaxSlots && uid_[slot] != 0;
    }
    // the slot was loaded on every rank: a fresh non-zero uid
    uint64_t Publish(int slot) {
        std::lock_guard<std::mutex> g(mu_);
        do {
            state_ = state_ * 6364136223846793005ULL + 1442695040888963407ULL;
        } while ((state_ >> 1) == 0);
        uid_[slot] = state_;
        refs_[slot] = 0;
        return uid_[slot];
    }
    // takes the slot out of service unless a pending or running request names it (-1: not loaded, 0: busy, 1: retired)
    int Retire(int slot) {
        std::lock_guard<std::mutex> g(mu_);
        if (slot < 0 || slot >= kMaxSlots || uid_[slot] == 0) return -1;
        if (refs_[slot] > 0) return 0;
        uid_[slot] = 0;
        return 1;
    }
    // held by LLMEngine::Execute for a step and by the backend while it loads or unloads: the device workers serve one of them at a time
    std::mutex& DeviceMutex() { return device_mu_; }

private:
    std::mutex mu_, device_mu_;
    uint64_t uid_[kMaxSlots] = {0};
    int64_t refs_[kMaxSlots] = {0};
    uint64_t state_ = 0x9e3779b97f4a7c15ULL;
};

}}  // namespace ppl::llm
