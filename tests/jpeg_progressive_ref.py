"""NumPy / pure-Python restatement of libjpeg's progressive Huffman decoder (jdphuff.c), the rule csrc/jpeg_progressive.hip follows bit for
bit.  Pillow (libjpeg-turbo) is the judge of this file (tests/test_jpeg_progressive_host.py); this file is the judge of the kernel and
provides its coefficient tap.  The marker walk and the scan validation are maf_yolo_amd.jpeg.parse(progressive=True) (tested on their own);
from its scan table to the coefficient array everything is restated here, and from the coefficients onward the IDCT, the upsampling and
the colour conversion are those of tests/jpeg_ref.py, imported.

  scans          jdphuff.c start_pass_phuff_decoder picks one of four routines per scan: Ss == 0 is a DC scan, Ah == 0 a first pass.  Each
                 scan decodes with the Huffman tables and the restart interval in force at ITS SOS marker (jdmarker.c get_dht / get_dri)
  geometry       jdinput.c per_scan_setup: a scan of all components is interleaved over the frame's MCU grid (per component v x h blocks,
                 row-major, as in baseline); a one-component scan has one block per MCU over ceil(comp_w / 8) x ceil(comp_h / 8) blocks of
                 the component's OWN sample dimensions, so the padding blocks of the frame's MCU grid never receive AC coefficients; the
                 restart interval counts the scan's own MCUs
  restarts       process_restart: bit reader realigned, DC predictions and EOBRUN reset to 0
  DC first       decode_mcu_DC_first: Huffman category s, diff = HUFF_EXTEND(get(s), s), coef[0] = (pred += diff) << Al
  DC refine      decode_mcu_DC_refine: one raw bit per block; if set coef[0] |= 1 << Al
  AC first       decode_mcu_AC_first: if EOBRUN > 0 the block is skipped and EOBRUN decremented; else symbols (r, s) from k = Ss: s != 0
                 places HUFF_EXTEND(get(s), s) << Al at k + r; s == 0, r == 15 (ZRL) skips 16; s == 0, r < 15 sets EOBRUN = (1 << r) +
                 get(r) - 1 and ends the block
  AC refine      decode_mcu_AC_refine: p1 = 1 << Al, m1 = -1 << Al.  If EOBRUN == 0, symbols (r, s): s must be 1 or 0; s == 1 reads a sign
                 bit (1: p1, 0: m1); s == 0, r < 15 sets EOBRUN = (1 << r) + get(r) and leaves the symbol loop; then (for s == 1 and ZRL)
                 the positions from k on are walked: an already NONZERO coefficient takes one correction bit, and if the bit is 1 and the
                 coefficient's p1 bit is not set yet, p1 (coefficient >= 0) or m1 (< 0) is added; a ZERO position counts down r and the
                 walk stops at the zero where r runs out, which is where the new coefficient goes.  If EOBRUN > 0 (just set, or from an
                 earlier block), every nonzero coefficient from k to Se takes its correction bit the same way and EOBRUN is decremented
  coefficients   JCOEF is a short: values wrap to int16; natural order through jutils.c jpeg_natural_order (J.ZIGZAG)

COUNTERS counts how often each hard branch was taken since reset_counters() (tests assert that the fixture set reaches every one).
"""
import numpy as np

import jpeg_ref as R
from maf_yolo_amd import jpeg as J

COUNTER_NAMES = ("ac_first_eobrun_gt1", "ac_first_zrl", "ac_refine_zrl", "correction_positive", "correction_negative", "ac_refine_new_coefficient",
                 "ac_refine_eobrun_tail_corrects", "restart_resets_eobrun")
COUNTERS = dict.fromkeys(COUNTER_NAMES, 0)
TRACE = None          # a list to receive (scan, interval, bit position of the extra bits in the unstuffed interval, r, block, run length) of every
                      # EOBr symbol with r > 0 of the AC first passes (tools/make_golden_jpeg_progressive.py finds the run it lengthens with it)


def reset_counters():
    for k in COUNTER_NAMES:
        COUNTERS[k] = 0


def _short(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _correct(blk, z, br, p1, m1):
    """One correction bit for the nonzero coefficient at natural position z -> 1 if it changed the coefficient."""
    v = int(blk[z])
    if br.bit() and (v & p1) == 0:
        blk[z] = _short(v + (p1 if v >= 0 else m1))
        COUNTERS["correction_positive" if v >= 0 else "correction_negative"] += 1
        return 1
    return 0


def coefficients(data, info=None):
    """Entropy decode of every scan -> (list of int16 [bh_c, bw_c, 64] natural-order coefficient arrays per component, padded to whole
    MCUs like jpeg_ref.coefficients, status word)."""
    d = J._bytes(data)
    info = info or J.parse(d, progressive=True)
    nc, hs, vs, mcux, mcuy, _ = J.geometry(info)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    coefs = [np.zeros((mcuy * v, mcux * h, 64), np.int16) for h, v in samp]
    zz = J.ZIGZAG.tolist()
    total_status = 0
    for si, sc in enumerate(info.scans):
        inter = len(sc.components) > 1
        if inter:
            gw, gh = mcux, mcuy
        else:
            ch, cv = samp[sc.components[0]]
            gw, gh = -(-(-(-info.width * ch // hs)) // 8), -(-(-(-info.height * cv // vs)) // 8)
        total = gw * gh
        ri = sc.restart_interval or total
        dc = sc.ss == 0
        tabs = None if dc and sc.ah else [R._canon(*sc.huffman[(0 if dc else 1, t)]) for t in (sc.td if dc else sc.ta)]
        p1, m1 = 1 << sc.al, -(1 << sc.al)
        eobrun = 0
        for k, (b0, b1) in enumerate(J._restart_ranges(d, sc.range, -(-total // ri))):
            br = R._Bits(d[b0:b1])
            if eobrun:
                COUNTERS["restart_resets_eobrun"] += 1
            pred, eobrun, status = [0] * len(sc.components), 0, 0
            for m in range(k * ri, min((k + 1) * ri, total)):
                my, mx = divmod(m, gw)
                if dc:
                    for j, c in enumerate(sc.components):
                        h, v = samp[c] if inter else (1, 1)
                        for by in range(v):
                            for bx in range(h):
                                blk = coefs[c][my * v + by, mx * h + bx]
                                if sc.ah == 0:                                   # decode_mcu_DC_first
                                    s = R._sym(br, tabs[j])
                                    if s is None or s > 16:
                                        status |= J.STATUS_BAD_CODE
                                        break
                                    pred[j] += R._extend(br.get(s), s) if s else 0
                                    blk[0] = _short(pred[j] << sc.al)
                                elif br.bit():                                   # decode_mcu_DC_refine
                                    blk[0] = _short(int(blk[0]) | p1)
                            if status:
                                break
                        if status:
                            break
                elif sc.ah == 0:                                                 # decode_mcu_AC_first
                    blk = coefs[sc.components[0]][my, mx]
                    if eobrun > 0:
                        eobrun -= 1
                        continue
                    kk = sc.ss
                    while kk <= sc.se:
                        rs = R._sym(br, tabs[0])
                        if rs is None:
                            status |= J.STATUS_BAD_CODE
                            break
                        r, s = rs >> 4, rs & 15
                        if s:
                            kk += r
                            if kk > sc.se:
                                status |= J.STATUS_BAD_INDEX if kk > 63 else J.STATUS_REFINE_PAST_SE
                                break
                            blk[zz[kk]] = _short(R._extend(br.get(s), s) << sc.al)
                            kk += 1
                        elif r == 15:
                            kk += 16
                            COUNTERS["ac_first_zrl"] += 1
                        else:
                            eobrun = (1 << r) + (br.get(r) if r else 0) - 1
                            if eobrun > 0:
                                COUNTERS["ac_first_eobrun_gt1"] += 1
                                if TRACE is not None:
                                    TRACE.append((si, k, br.pos - r, r, m, eobrun + 1))
                            break
                else:                                                            # decode_mcu_AC_refine
                    blk = coefs[sc.components[0]][my, mx]
                    kk = sc.ss
                    if eobrun == 0:
                        while kk <= sc.se:
                            rs = R._sym(br, tabs[0])
                            if rs is None:
                                status |= J.STATUS_BAD_CODE
                                break
                            r, s = rs >> 4, rs & 15
                            if s:
                                if s != 1:
                                    status |= J.STATUS_BAD_CODE
                                    break
                                s = p1 if br.bit() else m1
                            elif r != 15:
                                eobrun = (1 << r) + (br.get(r) if r else 0)
                                break
                            else:
                                COUNTERS["ac_refine_zrl"] += 1
                            while kk <= sc.se:
                                z = zz[kk]
                                if blk[z] != 0:
                                    _correct(blk, z, br, p1, m1)
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                kk += 1
                            if s:
                                if kk > sc.se:
                                    status |= J.STATUS_REFINE_PAST_SE
                                    break
                                blk[zz[kk]] = s
                                COUNTERS["ac_refine_new_coefficient"] += 1
                            kk += 1
                    if eobrun > 0 and not status:
                        changed = 0
                        while kk <= sc.se:
                            z = zz[kk]
                            if blk[z] != 0:
                                changed += _correct(blk, z, br, p1, m1)
                            kk += 1
                        if changed:
                            COUNTERS["ac_refine_eobrun_tail_corrects"] += 1
                        eobrun -= 1
                if status:
                    break
            if br.overrun:                                  # zeros past the interval's end were consumed: that is the fault, whatever they decoded to
                status = J.STATUS_SHORT_SCAN
            total_status |= status
    return coefs, total_status


def decode(data):
    """File bytes of a progressive (or, through jpeg_ref, a baseline) file -> uint8 [h, w, 3] BGR, what cv2.imread returns (EXIF rotation aside)."""
    d = J._bytes(data)
    info = J.parse(d, progressive=True)
    if info.scans is None:
        return R.decode(d)
    coefs, status = coefficients(d, info)
    if status:
        raise J.MafError("jpeg_progressive_ref: " + J.status_text(status))
    pl = [R.idct_plane(c, info.qtables[comp.tq]) for c, comp in zip(coefs, info.components)]
    w, h = info.width, info.height
    y = pl[0][:h, :w]
    if len(pl) == 1:
        return np.repeat(y[:, :, None], 3, 2)
    _, hs, vs, _, _, _ = J.geometry(info)
    return R.ycc_to_bgr(y, R.upsample(pl[1], w, h, hs, vs), R.upsample(pl[2], w, h, hs, vs))
