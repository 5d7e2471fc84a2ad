#include "guide_cache.h"

#include "ppl/common/log.h"

using namespace ppl::common;

namespace ppl { namespace llm {

GuideCache::~GuideCache() {
    for (int32_t i = 0; i < PostProcessor::kGuideMaxSlots; ++i)
        if (!slots_[i].key.empty()) engine_->UnloadGuide(i);
}

// the first guided request: the vocabulary goes to the backend, once; a backend that refused it stays refused
bool GuideCache::SendVocab() {
    if (vocab_sent_ == 0) {
        std::string bytes, blob;
        std::vector<int64_t> offsets(1, 0);
        for (int32_t t = 0; t < vocab_size_; ++t) {
            tokenizer_->TokenBytes(t, &bytes);
            blob += bytes;
            offsets.push_back((int64_t)blob.size());
        }
        const RetCode rc = engine_->SetGuideVocab((const uint8_t*)blob.data(), offsets.data(), vocab_size_);
        vocab_sent_ = rc == RC_SUCCESS ? 1 : -1;
        if (rc != RC_SUCCESS) LOG(ERROR) << "SetGuideVocab failed: " << GetRetCodeStr(rc);
    }
    return vocab_sent_ > 0;
}

int32_t GuideCache::Acquire(Kind kind, const std::string& text, const std::vector<int32_t>& end_tokens, std::string* err, RetCode* errcode) {
    const bool wide = kind == Kind::kJsonSchema;
    const auto refuse = [&](RetCode code, const std::string& msg) {
        *errcode = code;
        *err = (wide ? "guide_json_schema: " : "guide_regex: ") + msg;
        return -1;
    };
    if (!engine_->HasGuides()) return refuse(RC_UNSUPPORTED, "the backend's post processor has no GuideEdit");
    std::string bytes;
    if (!tokenizer_ || !tokenizer_->TokenBytes(0, &bytes))
        return refuse(RC_UNSUPPORTED, "needs a tokenizer that knows the bytes of its tokens (TokenBytes)");
    if (!SendVocab()) return refuse(RC_OTHER_ERROR, "the backend refused the vocabulary");
    if ((int32_t)end_tokens.size() > PostProcessor::kLogitStopMax)
        return refuse(RC_INVALID_VALUE, "more than " + std::to_string(PostProcessor::kLogitStopMax) + " end tokens");
    for (int32_t t : end_tokens)
        if (t < 0 || t >= vocab_size_) return refuse(RC_INVALID_VALUE, "end token [" + std::to_string(t) + "] outside the vocabulary");

    std::string key(1, wide ? 'J' : 'R');
    key += text;
    key.push_back('\0');
    for (int32_t t : end_tokens) key += std::to_string(t) + ",";
    const int32_t n = PostProcessor::kGuideMaxSlots;
    for (int32_t i = 0; i < n; ++i)
        if (slots_[i].key == key) {
            ++slots_[i].refs;
            slots_[i].last_use = ++clock_;
            return i;
        }
    GuideDfa dfa;
    GuideDfa16 dfa16;
    *errcode = RC_INVALID_VALUE;
    if (!(wide ? CompileGuideJsonSchema(text, &dfa16, err) : CompileGuideRegex(text, &dfa, err))) return -1;
    int32_t pick = -1;
    for (int32_t i = 0; i < n && pick < 0; ++i)
        if (slots_[i].key.empty()) pick = i;
    if (pick < 0) {  // evict the idle slot that was used longest ago
        for (int32_t i = 0; i < n; ++i)
            if (slots_[i].refs == 0 && (pick < 0 || slots_[i].last_use < slots_[pick].last_use)) pick = i;
        if (pick < 0) return refuse(RC_OTHER_ERROR, "all " + std::to_string(n) + " guide slots are held by running requests");
        const RetCode rc = engine_->UnloadGuide(pick);
        if (rc != RC_SUCCESS) return refuse(RC_OTHER_ERROR, "UnloadGuide failed: " + std::string(GetRetCodeStr(rc)));
        slots_[pick] = Slot();
    }
    const RetCode rc = wide ? engine_->LoadGuide16(pick, dfa16, end_tokens) : engine_->LoadGuide(pick, dfa, end_tokens);
    if (wide && rc == RC_UNSUPPORTED) return refuse(RC_UNSUPPORTED, "the backend's post processor has no LoadGuide16");
    if (rc == RC_INVALID_VALUE)
        return refuse(RC_INVALID_VALUE, std::string("some state of the ") + (wide ? "schema" : "pattern") +
                                            "'s automaton allows no token of the vocabulary");
    if (rc != RC_SUCCESS) return refuse(RC_OTHER_ERROR, std::string(wide ? "LoadGuide16" : "LoadGuide") + " failed: " + GetRetCodeStr(rc));
    slots_[pick].key = key;
    slots_[pick].wide = wide;
    slots_[pick].dfa = std::move(dfa);
    slots_[pick].dfa16 = std::move(dfa16);
    slots_[pick].refs = 1;
    slots_[pick].last_use = ++clock_;
    return pick;
}

void GuideCache::Release(int32_t slot) {
    if (slot < 0 || slot >= PostProcessor::kGuideMaxSlots) return;
    if (slots_[slot].refs > 0) --slots_[slot].refs;
}

}}  // namespace ppl::llm
