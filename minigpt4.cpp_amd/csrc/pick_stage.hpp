// THE staging block of a device pick (k_pen_pick: PickStage<PenRow, int>, k_constrain_pick: <ConRow, int>, k_sample_rows: <SampleRow, SampleOut>), N rows at most.
// One device and one pinned block of the same layout -- [N] Row descriptors, then the rows' penalty tables back to back, N * PEN_TABLE_MAX PenEntry (penalty.hpp; a
// descriptor's `off` counts entries from the first table) -- so a call's descriptors and tables travel in ONE upload; [N] Out on the device with its pinned mirror, the
// landing place of the results; the event recorded behind their copy, for a caller that awaits them while later work runs.  Only this type knows the layout.
// alloc(): all five handles or none, at the feature's first use; reset_all / abandon_all take it like a handle.  The pinned blocks are the caller's to keep free: it has
// synchronised since the last upload or fetch was queued before it writes rows() / entries() or reads out_h().
#pragma once
#include "owned.hpp"
#include "penalty.hpp"

namespace mg4 {

template <typename Row, typename Out, int N> class PickStage {
    static constexpr size_t HEAD = (size_t)N * sizeof(Row), BYTES = HEAD + (size_t)N * PEN_TABLE_MAX * sizeof(PenEntry);
    static_assert(HEAD % alignof(PenEntry) == 0 && HEAD % 16 == 0, "the tables start aligned behind the descriptors");
    DevPtr<uint8_t> d_; PinPtr<uint8_t> h_; DevPtr<Out> out_d_; PinPtr<Out> out_h_; OwnedEvent ev_;
public:
    explicit operator bool() const { return d_ != nullptr; }
    void alloc() {
        if (d_) return;
        DevPtr<uint8_t> d(BYTES); PinPtr<uint8_t> h(BYTES); DevPtr<Out> out_d((size_t)N * sizeof(Out)); PinPtr<Out> out_h((size_t)N * sizeof(Out)); OwnedEvent ev(0);
        d_ = std::move(d); h_ = std::move(h); out_d_ = std::move(out_d); out_h_ = std::move(out_h); ev_ = std::move(ev);
    }
    void reset() noexcept { reset_all(d_, h_, out_d_, out_h_, ev_); }
    void abandon() noexcept { abandon_all(d_, h_, out_d_, out_h_, ev_); }
    Row *rows() const { return h_.template as<Row>(); }                                    // pinned: descriptor r
    PenEntry *entries() const { return reinterpret_cast<PenEntry *>(h_ + HEAD); }         // pinned: the tables
    const Row *d_rows() const { return d_.template as<const Row>(); }
    const PenEntry *d_entries() const { return reinterpret_cast<const PenEntry *>(d_ + HEAD); }
    Out *out_h() const { return out_h_; }
    Out *out_d() const { return out_d_; }
    hipEvent_t event() const { return ev_; }
    // every descriptor and the first n_ent table entries, one copy
    void upload(size_t n_ent, hipStream_t s) { HIP_CHECK(hipMemcpyAsync(d_, h_, HEAD + n_ent * sizeof(PenEntry), hipMemcpyHostToDevice, s)); }
    // the first n * bytes_per_row bytes of the results into the pinned mirror, and the event behind them
    void fetch(int n, size_t bytes_per_row, hipStream_t s) {
        HIP_CHECK(hipMemcpyAsync(out_h_, out_d_, (size_t)n * bytes_per_row, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(ev_, s));
    }
};

}  // namespace mg4
