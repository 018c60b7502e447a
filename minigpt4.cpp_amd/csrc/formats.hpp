// Readers for the two on-disk formats the reference consumes (host only, no GPU dependency).
//   format A: MiniGPT-4 vision container, "ggml" magic v1   (reference reader minigpt4.cpp:1478-1596, writer convert.py:74-180)
//   format B: Vicuna LLM file, GGJT v3                        (read by llama.cpp behind minigpt4.cpp:1783; layout SURVEY.md 2.5)
//   format B': the same model as a GGUF v2/v3 file (what current llama.cpp converters write) -- mapped onto the GGJT view below
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace mg4 {

struct MappedFile {
    int fd = -1;
    const uint8_t *data = nullptr;
    size_t size = 0;
    bool open(const std::string &path);
    void close();
    ~MappedFile() { close(); }
    MappedFile() = default;
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};

struct TensorMeta {
    std::string name;
    int type = -1;                 // ggml_type numbering
    std::vector<int64_t> ne;       // innermost first
    size_t offset = 0, nbytes = 0;
    int64_t nelements() const { int64_t n = 1; for (auto v : ne) n *= v; return n; }
};

struct VisionFile {
    MappedFile mf;
    int version = 0, ftype = 0;
    std::string config_json;
    std::vector<std::string> model_order;
    std::map<std::string, std::map<std::string, TensorMeta>> models;
    int load(const std::string &path);   // returns MiniGPT4Error
    const TensorMeta *find(const std::string &model, const std::string &name) const;
    int64_t config_int(const std::string &key, int64_t dflt) const;   // first occurrence of "key": <int> in the JSON config
};

struct LLMFile {
    MappedFile mf;
    uint32_t n_vocab = 0, n_embd = 0, n_mult = 0, n_head = 0, n_layer = 0, n_rot = 0, ftype = 0;
    std::vector<std::string> pieces;
    std::vector<float> scores;
    std::map<std::string, TensorMeta> tensors;
    uint32_t n_ff_explicit = 0;                                   // GGUF files state the feed-forward width; GGJT files derive it from n_mult
    int load(const std::string &path, bool vocab_only = false);   // returns MiniGPT4Error (LoadLanguageModel on malformed input); GGJT v3 or GGUF v2/v3 by magic
    int load_gguf(bool vocab_only);                               // mf already mapped
    uint32_t n_ff() const { return n_ff_explicit ? n_ff_explicit : ((2 * (4 * n_embd) / 3 + n_mult - 1) / n_mult) * n_mult; }
    const TensorMeta *find(const std::string &name) const { auto it = tensors.find(name); return it == tensors.end() ? nullptr : &it->second; }
};

// A LoRA adapter as convert_lora_to_gguf.py writes it (GGUF v2 / v3): general.type = "adapter", adapter.type = "lora", adapter.lora.alpha, tensors
// blk.N.<target>.weight.lora_a (ggml ne = (n_in, r)) / .lora_b (ne = (r, n_out)), F16 or F32.  Any subset of the seven targets and of the layers; one rank 1..64 per file.
constexpr int LORA_FILE_RANK_MAX = 64;
enum AdapterRefusal : int { ADAPTER_OK = 0, ADAPTER_BAD_TYPE = 1, ADAPTER_UNPAIRED = 2, ADAPTER_BAD_SHAPE = 3, ADAPTER_BAD_RANK = 4, ADAPTER_BAD_TENSOR_TYPE = 5, ADAPTER_MALFORMED = 6 };
enum AdapterTarget : int { AT_Q = 0, AT_K, AT_V, AT_O, AT_GATE, AT_DOWN, AT_UP, AT_COUNT };   // attn_q, attn_k, attn_v, attn_output, ffn_gate (w1), ffn_down (w2), ffn_up (w3)
struct AdapterFile {
    MappedFile mf;
    float alpha = 0.0f;
    int rank = 0, n_tensors = 0, n_layers = 0;                    // layers with at least one pair
    unsigned target_mask = 0;                                     // bit AdapterTarget
    bool any_f32 = false;                                         // some tensor is F32: the fp16 device copy rounds it
    struct Pair { const TensorMeta *a = nullptr, *b = nullptr; };
    std::map<std::string, TensorMeta> tensors;
    std::map<int, std::array<Pair, AT_COUNT>> layers;             // layer index -> its pairs
    // ADAPTER_OK, or the refusal with last_error "adapter file: ..." (shapes are checked among the file's own tensors: the targets that share an input or an output
    // width must agree; Engine::adapter_load checks them against the model)
    int load(const std::string &path);
    size_t device_bytes() const;                                  // fp16 A and B images with the rank padded to a multiple of 16
    int rank_padded() const { return (rank + 15) / 16 * 16; }
};

// llama.cpp (master-31cfbb1) SentencePiece-style tokenizer over the file vocab: UTF-8 split, greedy best-score bigram merges,
// byte fallback (id = byte + 3).  Reference call site: minigpt4.cpp:2389.
struct Tokenizer {
    const std::vector<std::string> *pieces = nullptr;
    const std::vector<float> *scores = nullptr;
    std::unordered_map<std::string, int> token_to_id;
    void init(const LLMFile &f);
    std::vector<int> tokenize(const std::string &text, bool add_bos) const;
};

}  // namespace mg4
