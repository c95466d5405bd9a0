"""liba52 channel flags (a52dec-0.7.5-cvs/include/a52.h:40-54)."""
A52_CHANNEL = 0
A52_MONO = 1
A52_STEREO = 2
A52_3F = 3
A52_2F1R = 4
A52_3F1R = 5
A52_2F2R = 6
A52_3F2R = 7
A52_CHANNEL1 = 8
A52_CHANNEL2 = 9
A52_DOLBY = 10
A52_CHANNEL_MASK = 15
A52_LFE = 16
A52_ADJUST_LEVEL = 32

NFCHANS = (2, 1, 2, 3, 3, 4, 4, 5, 1, 1, 2)


def out_channels(flags):
    return NFCHANS[flags & A52_CHANNEL_MASK] + (1 if flags & A52_LFE else 0)

# d_status bits of the batched decoder (include/ac3mi.h)
STATUS_REFUSED = 0x100      # a52_syncinfo / a52_frame refused the frame
STATUS_REUSE0 = 0x200
STATUS_CRC1 = 0x400         # CRC-16 of bytes [2, 2 fs58) is not 0 (ac3mi_set_decode_crc 1 / 2)
STATUS_CRC2 = 0x800         # CRC-16 of bytes [2 fs58, 2 fs) is not 0
# ac3mi_set_decode_crc modes
CRC_OFF, CRC_REPORT, CRC_CONCEAL = 0, 1, 2
# ac3mi_crc_check_batch verdict bits
VERDICT_CRC1, VERDICT_CRC2, VERDICT_NOT_SUMMED = 1, 2, 0x80
# ac3mi_bsi_info: verdict bits and the bits of `present`
BSI_NOT_READ, BSI_OVERRUN = 0x80, 0x40
BSI_PRESENT = {"compre": 0x001, "langcode": 0x002, "audprodie": 0x004, "compr2e": 0x008, "langcod2e": 0x010,
               "audprodi2e": 0x020, "timecod1e": 0x040, "timecod2e": 0x080, "addbsie": 0x100}
# ac3mi_set_encode_metadata_source modes
MD_SOURCE_CONTEXT, MD_SOURCE_FOLLOW = 0, 1
# ac3mi_set_encode_drc_source modes
DRC_SOURCE_CONTEXT, DRC_SOURCE_FOLLOW = 0, 1
# ac3mi_set_encode_dynrng_frames: bit 8 of a compr word of the array says that the word is sent (compre / compr2e)
COMPR_SENT = 0x100
