// rcf_streams.h -- the streams a channel can be read as, one row each, and the integer rules every reader of them shares.
// Nothing of HIP and nothing of the host state in here: g++ alone compiles it (tests/native/stream_table_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/rcf.h"

namespace rcfx {

// One row per stream: its index is the stream's `kind` inside the library, `what` its name in the ABI.
struct StreamKind {
    int what;               // RCF_READ_* / RCF_HARD_*
    uint32_t item_w;        // 4-byte words per item
    bool u32;               // items are uint32 (else float32 / cf32)
    bool counted;           // the stream ends at a device counter of its stage (else at the channel's `produced`)
    bool pumped;            // the pump delivers it
    const char *refusal;    // RCF_ESTATE: what a channel without that ring says (%d: the channel)
};
enum : int { kIq, kFm, kAgc, kSym, kClock, kAudio, kCostas, kFsk4, kHardBits, kHardSync, kTsbk, kStreamKinds };
constexpr StreamKind kStreams[kStreamKinds] = {
    {RCF_READ_IQ,     2, false, false, true,  "channel %d exposes its discriminator only (rcf_chan_set_fm_only)"},
    {RCF_READ_FM,     1, false, false, true,  "channel %d has no discriminator ring"},
    {RCF_READ_AGC,    2, false, false, true,  "channel %d has no AGC"},
    {RCF_READ_SYM,    1, false, false, true,  "channel %d has no fm filter"},
    {RCF_READ_CLOCK,  1, false, true,  true,  "channel %d has no symbol clock"},
    {RCF_READ_AUDIO,  1, false, true,  true,  "channel %d has no audio chain"},
    {RCF_READ_COSTAS, 1, false, true,  true,  "channel %d has no Gardner / Costas stage"},
    {RCF_READ_FSK4,   1, false, true,  true,  "channel %d has no C4FM symbol loop (rcf_chan_fsk4)"},
    {RCF_HARD_BITS,   1, true,  true,  false, "channel %d has no slicer (rcf_chan_slicer)"},
    {RCF_HARD_SYNC,   1, true,  true,  false, "channel %d has no slicer (rcf_chan_slicer)"},
    {RCF_HARD_TSBK,   8, true,  true,  false, "channel %d has no TSBK stage (rcf_chan_tsbk)"},
};
// the row of `what`; -1: no such stream (3 .. 15 stay refused)
constexpr int stream_kind(int what)
{
    for (int k = 0; k < kStreamKinds; ++k)
        if (kStreams[k].what == what) return k;
    return -1;
}
static_assert(stream_kind(RCF_READ_AUDIO) == kAudio && stream_kind(RCF_HARD_SYNC) == kHardSync && stream_kind(RCF_HARD_TSBK) == kTsbk, "the rows stand in the enum's order");
// That table and stream_kind are also the pump's: its two entry points take a `what` through them and refuse what they do not
// find or find unpumped, and its slots hold a row's index.  A stream that only the readers carry -- none of the pump's code
// knows its items -- is added BEHIND the table, so that nothing the pump or a consumer of the table compiled against moves:
// the readers' kinds go on where the table's end, read_kind / read_row are their stream_kind / kStreams.
// kReadKinds is where the rows ended when the first of them (49) came, and stays there -- a consumer compiled against it sees
// what it saw; rows added since go on behind it, and kAllReadKinds ends them all.  A new stream takes a number that was never
// refused by name: 50 stands in the suite as the readers' example of "no such stream", so the OSW stage's is 51.
// kAllReadKinds in turn is where they ended when the P25 voice stage's row came (the suite pins it as it pins kReadKinds, and
// 52 beside 50 as no stream: the row's number is 53); kReadKindsEnd ends them all now, and the readers' loops run to it.
enum : int { kEdacs = kStreamKinds, kReadKinds, kOsw = kReadKinds, kAllReadKinds, kP25lc = kAllReadKinds, kReadKindsEnd };
constexpr StreamKind kReadOnlyStreams[kReadKindsEnd - kStreamKinds] = {
    {RCF_HARD_EDACS,  8, true,  true,  false, "channel %d has no EDACS stage (rcf_chan_edacs)"},
    {RCF_HARD_OSW,    8, true,  true,  false, "channel %d has no OSW stage (rcf_chan_osw)"},
    {RCF_HARD_P25LC,  8, true,  true,  false, "channel %d has no P25 voice stage (rcf_chan_p25lc)"},
};
constexpr const StreamKind &read_row(int kind) { return kind < kStreamKinds ? kStreams[kind] : kReadOnlyStreams[kind - kStreamKinds]; }
// the readers' kind of `what`: a row of the table, or one behind it; -1: no such stream
constexpr int read_kind(int what)
{
    if (stream_kind(what) >= 0) return stream_kind(what);
    for (int k = kStreamKinds; k < kReadKindsEnd; ++k)
        if (read_row(k).what == what) return k;
    return -1;
}
static_assert(read_kind(RCF_HARD_EDACS) == kEdacs && stream_kind(RCF_HARD_EDACS) == -1 && read_kind(RCF_HARD_TSBK) == kTsbk && !read_row(kEdacs).pumped,
              "the readers' rows go on behind the table; the pump finds none of them");
static_assert(read_kind(RCF_HARD_OSW) == kOsw && stream_kind(RCF_HARD_OSW) == -1 && !read_row(kOsw).pumped && read_kind(50) == -1, "likewise");
static_assert(read_kind(RCF_HARD_P25LC) == kP25lc && stream_kind(RCF_HARD_P25LC) == -1 && !read_row(kP25lc).pumped && read_kind(52) == -1, "likewise");

// A reader that has fallen more than a ring of `cap` items behind lost what the ring overwrote: its cursor is raised to the
// oldest item the ring still holds (the ring holds the cap items before `newest`).  Returns how many items [*cursor, end) it
// may take, at most max.
inline int64_t lag_clamp(int64_t cap, int64_t *cursor, int64_t newest, int64_t end, int64_t max)
{
    if (*cursor < newest - cap) *cursor = newest - cap;
    const int64_t n = end - *cursor < max ? end - *cursor : max;
    return n > 0 ? n : 0;
}
// a counted stream's items so far: ceil(counter * interp / decim) (gather_counted_kernel computes the same)
inline int64_t count_end(int64_t counter, uint32_t interp, uint32_t decim)
{
    return interp == decim ? counter : (counter * (int64_t)interp + (int64_t)decim - 1) / (int64_t)decim;
}
// the most a steady-state gather of the pump takes after a block of n_k stage inputs: n_k + 1 symbols of a loop (interp =
// decim = 1), ceil(n_k interp / decim) + 1 audio samples
inline int64_t steady_bound(int64_t n_k, uint32_t interp, uint32_t decim) { return count_end(n_k, interp, decim) + 1; }
// a plain slot of the pump: of the n items from *cursor on, those a host ring of `room` items cannot hold are skipped
inline int64_t ring_room(int64_t *cursor, int64_t n, int64_t room)
{
    if (n > room) { *cursor += n - room; n = room; }
    return n;
}

}  // namespace rcfx
