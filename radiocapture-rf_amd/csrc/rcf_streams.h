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
// find or find unpumped.  (rcf_pump_subscribe_hard, the pump's third, takes the counted uint32 streams -- rows 32, 33 and 48 and
// the rows behind the table -- through read_kind, and a slot holds a reader's kind.)  A stream that only the readers carry -- none
// of the code compiled against the table knows its items -- is added BEHIND the table, so that nothing the pump or a consumer of the table compiled against moves:
// the readers' kinds go on where the table's end, read_kind / read_row are their stream_kind / kStreams.
// kReadKinds is where the rows ended when the first of them (49) came, and stays there -- a consumer compiled against it sees
// what it saw; rows added since go on behind it, and kAllReadKinds ends them all.  A new stream takes a number that was never
// refused by name: 50 stands in the suite as the readers' example of "no such stream", so the OSW stage's is 51.
// kAllReadKinds in turn is where they ended when the P25 voice stage's row came (the suite pins it as it pins kReadKinds, and
// 52 beside 50 as no stream: the row's number is 53); kReadKindsEnd ends them all now, and the readers' loops run to it.
// kReadKindsEnd in turn is where they ended when the capture stage's two rows came (rcf_chan_capture; the suite pins it too):
// 24, the first row behind the table that is not uint32 -- counted cf32, which rcf_pump_subscribe admits by name, as
// stream_kind and the table do not move --, and 56, its records, which rcf_pump_subscribe_hard delivers.  kReadRowsEnd ends
// them all now.  read_kind, too, stays what its consumers compiled against -- the suite walks it over 0 .. 60 and pins the
// streams it finds --: it goes on ending at kReadKindsEnd, and the readers and the pump look a `what` up with row_kind, which
// is read_kind and the rows behind kReadKindsEnd.
enum : int { kEdacs = kStreamKinds, kReadKinds, kOsw = kReadKinds, kAllReadKinds, kP25lc = kAllReadKinds, kReadKindsEnd,
             kCapture = kReadKindsEnd, kCaptureRec, kReadRowsEnd };
constexpr StreamKind kReadOnlyStreams[kReadRowsEnd - kStreamKinds] = {
    {RCF_HARD_EDACS,  8, true,  true,  false, "channel %d has no EDACS stage (rcf_chan_edacs)"},
    {RCF_HARD_OSW,    8, true,  true,  false, "channel %d has no OSW stage (rcf_chan_osw)"},
    {RCF_HARD_P25LC,  8, true,  true,  false, "channel %d has no P25 voice stage (rcf_chan_p25lc)"},
    {RCF_READ_CAPTURE, 2, false, true, true,  "channel %d has no capture stage (rcf_chan_capture)"},
    {RCF_HARD_CAPTURE, 8, true,  true,  false, "channel %d has no capture stage (rcf_chan_capture)"},
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
// the row of `what` among ALL rows: what the readers and the pump's subscriptions take; -1: no such stream
constexpr int row_kind(int what)
{
    if (read_kind(what) >= 0) return read_kind(what);
    for (int k = kReadKindsEnd; k < kReadRowsEnd; ++k)
        if (read_row(k).what == what) return k;
    return -1;
}
static_assert(read_kind(RCF_HARD_EDACS) == kEdacs && stream_kind(RCF_HARD_EDACS) == -1 && read_kind(RCF_HARD_TSBK) == kTsbk && !read_row(kEdacs).pumped,
              "the readers' rows go on behind the table; the pump finds none of them");
static_assert(read_kind(RCF_HARD_OSW) == kOsw && stream_kind(RCF_HARD_OSW) == -1 && !read_row(kOsw).pumped && read_kind(50) == -1, "likewise");
static_assert(read_kind(RCF_HARD_P25LC) == kP25lc && stream_kind(RCF_HARD_P25LC) == -1 && !read_row(kP25lc).pumped && read_kind(52) == -1, "likewise");
static_assert(row_kind(RCF_READ_CAPTURE) == kCapture && row_kind(RCF_HARD_CAPTURE) == kCaptureRec && read_kind(RCF_READ_CAPTURE) == -1 &&
              read_kind(RCF_HARD_CAPTURE) == -1 && read_row(kCapture).pumped && !read_row(kCaptureRec).pumped && row_kind(21) == -1 &&
              row_kind(50) == -1 && row_kind(52) == -1 && row_kind(RCF_HARD_P25LC) == kP25lc,
              "likewise; the captured stream is the one row behind the table that rcf_pump_subscribe delivers");

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
// A slot of the pump is out_cap x 8 bytes whatever it delivers; its host ring holds slot_items() of the stream's items: out_cap
// of up to 8 bytes (a 4-byte stream uses half the slot), out_cap / 4 of the 32-byte records.  Both are powers of two
inline int64_t slot_items(int kind, int64_t out_cap) { return read_row(kind).item_w <= 2 ? out_cap : out_cap * 2 / (int64_t)read_row(kind).item_w; }
// The most a steady-state gather of a slot of rcf_pump_subscribe_hard takes after a block of n_k channel outputs; bps = the
// slicer's bits per symbol (1, 2).  A symbol loop makes at most n_k + 1 symbols of them (steady_bound), so the slicer's whole
// words cover at most dW = n_k + 1 + (32 / bps - 1) more symbols than before the block: the unfinished word may have lacked
// one symbol.  Every frame decoder DECIDES a frame in the first block whose whole words reach a threshold that lies a fixed
// distance behind the frame's start (rcf.h: s + 384, s + 888, s + 288, pos + 84 or h0 + 92), so the frames of a block are those
// with a threshold among dW consecutive symbols, and the framing rule says how close two thresholds can lie:
//   words   ceil(n_k bps / 32) + 1       (n_k + 1 symbols behind an unfinished word of at most 32 - bps bits)
//   hits    n_k + 1                      (one item per symbol at most: the two polarities' ranges of dist do not meet)
//   TSBK    (n_k + 15) / 24 + 3          accepted hits lie >= 24 dibits apart, dW = n_k + 16.  A frame cut d dibits behind its start
//                                        gives 1 record for d < 259, 2 for d < 359, else 3 -- never more than d / 24 --, so all
//                                        frames but the block's last give at most (dW - 1) / 24 together, and the last at most 3
//   P25LC   (n_k + 15) / 24 + 1          the same accept rule, one record per frame
//   EDACS   (n_k + 31) / 288 + 1         accepted hits lie >= 288 bits apart, dW = n_k + 32, one record per frame
//   OSW     (n_k + 31) / 76 + 1          a packet's threshold is its sync position + 84 (step A) or + 92 (step B), the next
//                                        packet's sync position lies >= 84 bits on: thresholds >= 76 bits apart, dW = n_k + 32
// A stage that has more than this ready (a backlog behind a loss, say) is held to the bound by the gather kernel; the rest
// leaves with the next block.  -1: not a hard stream
inline int64_t hard_bound(int kind, int64_t n_k, int bps)
{
    if (n_k < 0) n_k = 0;
    switch (kind) {
    case kHardBits: return (n_k * bps + 31) / 32 + 1;
    case kHardSync: return n_k + 1;
    case kTsbk:     return (n_k + 15) / 24 + 3;
    case kP25lc:    return (n_k + 15) / 24 + 1;
    case kEdacs:    return (n_k + 31) / 288 + 1;
    case kOsw:      return (n_k + 31) / 76 + 1;
    default:        return -1;
    }
}
// The capture stage's two streams (rcf_chan_capture) after a block of n_k channel outputs.  The writer decides at most as
// many samples as the detector saw -- exactly as many once it runs pre behind --, so a block adds at most n_k captured
// samples.  Records: a block's events lie among n_k consecutive decided samples.  An OPEN and its CLOSE lie at least
// pre + hang + 1 apart (one open sample keeps that many), a CLOSE and the next OPEN at least 1 (two keyings pre + hang + 1
// apart leave one sample out), so two records cost pre + hang + 2 samples: E records span at least
// floor((E - 1) / 2) (pre + hang + 2) <= n_k - 1, E <= 2 floor((n_k - 1) / (pre + hang + 2)) + 2.  One window per attachment may be
// shorter -- the one whose lead-in is clipped at the attach point, hang + 1 at the least --, which the + 4 below covers
inline int64_t capture_bound(int64_t n_k) { return n_k < 0 ? 0 : n_k; }
inline int64_t capture_rec_bound(int64_t n_k, int64_t pre, int64_t hang)
{
    if (n_k < 0) n_k = 0;
    return 2 * (n_k / (pre + hang + 2)) + 4;
}
// a plain slot of the pump: of the n items from *cursor on, those a host ring of `room` items cannot hold are skipped
inline int64_t ring_room(int64_t *cursor, int64_t n, int64_t room)
{
    if (n > room) { *cursor += n - room; n = room; }
    return n;
}

}  // namespace rcfx
