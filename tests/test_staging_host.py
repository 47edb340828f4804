"""maf_yolo_amd/staging.py, the scaffold the image codecs and resizers share, on the host (no GPU):
* the blobs jpeg.build_blob / fill_blob and png.build_blob / fill_blob write for every golden file (each alone, and each set as one batch)
  hash to the SHA-256 digests below.  The digests were recorded from the commit BEFORE these modules moved onto staging.py (the hand-written
  layout code of each), never from the code under test: they pin the blob bytes across the move.  A change that is meant to alter a blob
  has to say so and record new digests from a reviewed build;
* blob_layout / write_blob: aligned, ordered, non-overlapping offsets and a round trip;
* checked_library: a size that is off by one raises MafError("... rebuild"), a key is checked once when it passes and again after it failed;
* file_bytes, file_name, status_text: what the copies in jpeg.py / png.py / frames.py returned;
* frame_list as far as CPU tensors reach, in both callers' wording.
"""
import hashlib
import importlib
import pathlib

import numpy as np
import pytest
import torch

from maf_yolo_amd import jpeg as J, jpeg_encode as E, png as P, staging as S
from maf_yolo_amd.lib import MafError

LB = importlib.import_module("maf_yolo_amd.letterbox")        # the package's `letterbox` is the function

# "*": the set's file_* entries, sorted by name, as one call
JPEG_CASES = {
    'grad_q75_17x33_s0': '69e9d0ecffe21cbd7ee197ff9f966ecb70633823b4f3565add85c601d5850b5e',
    'grad_q75_17x33_s1': '962e3df8ab7c785358cb4509e4f8df7993913503f3f667a4193d8bc410da1c79',
    'grad_q75_17x33_s2': '8fa38e2d07e6b7cbe89ce43026329045327e2212227ee835879e192cee4a0388',
    'grad_q75_1x1_s0': 'f7c4243a8c06d6f23c128729bba4da516df096ecc44ba68c212d1f9dcad477dd',
    'grad_q75_1x1_s1': 'a2759565a4ef7ae3352e49fb00d814f0b055c9a47607cf102dc0e898c4f6ab1b',
    'grad_q75_1x1_s2': '2c6a37a4f991f4963c2db277bb3c43e79e19e8b645c2abe56c07b05795e82a34',
    'grad_q75_48x64_s0': '15c2183927554aab19602652aa9277a11d3c719983566d01e6bda17f4868553d',
    'grad_q75_48x64_s1': '7fe4fa2e194684aaea13839211e100f048f84f6f5c88ee1c143974fbf24575d1',
    'grad_q75_48x64_s2': 'e8bbbe838b3c3a03b4bff4d1ce7a0c6ed0862340f4195fcf3e9c2bf5fd38a896',
    'grad_q75_75x100_s0': '60abd7cc71959dc960dbf4c848e07d6a9352e2763b675f140f0490e889c4c396',
    'grad_q75_75x100_s1': '1711c771cd1373c919b008215ed6eb2f3cd1847c37077f068d2a7431f9bc0b31',
    'grad_q75_75x100_s2': '3a178ba38f01643a75439d00543f47ff060ec6b532bb804777049b28e207f44e',
    'grad_q75_7x9_s0': '11b4c3e1c972fbafd6dc3b42229ba89981fb2f0b92e223d4304ec60f4d42a5b8',
    'grad_q75_7x9_s1': 'e9165299a082857d0e166c1ba516717da71da6d308f8cbdc5960907e92cf34ac',
    'grad_q75_7x9_s2': 'ae2185f26c78711d7461405a3a5e8fd1892b320ee2b473526c6b3823069a626e',
    'grad_q75_8x8_s0': 'ae7ee31c7107414f45aae5fb636e224a659cbae0e21e731f06fb64df180716c7',
    'grad_q75_8x8_s1': 'c1d864f3c213c33da71456cf0924b6688fe9e300f211cf8a9c0affd8f3ef9ad9',
    'grad_q75_8x8_s2': '5c2f5b807eb4f3a18b33df6893b00aeaf8f3e1f612cb4947d46ac105574ca76c',
    'grad_q75_rst2_17x33_s0': '28d0f73392cc6af2bd472cb05f322a1a6221f9a9b26a3582d026561e85362910',
    'grad_q75_rst2_17x33_s1': '32e2a024697f7c8ea14dff17d2ed08d52f6927b6c61abe184697677cd3505cc4',
    'grad_q75_rst2_17x33_s2': '80cf11bc62c641c97da0a849254da362b8bc1dfa6eb35e73116c12489bffca80',
    'grad_q75_rstrow_48x64_s0': '471894f1caf07bd174ee3ba9eb32de65d803eb14b1b30a278260f63c4cdab6f5',
    'grad_q75_rstrow_48x64_s1': '1d96bc9879909e60aa527b0c426185da24e34ecee8d025f58198ea833b99c78c',
    'grad_q75_rstrow_48x64_s2': 'e7bce5af3f392cc720d6d6e1f0e42ed6f40726860df1a22e85278e845cdfc4d9',
    'gray_q75_17x33': '60889737ff018cbb26f62ebfb566c451904594ecf0748f8aee6df48374dad634',
    'noise_q100_17x33_s0': '54c75e4fb6d70e25e3ef2a07c693ed679b65cc791a08fce0cf5e7a0357c7c8dc',
    'noise_q100_17x33_s1': '799c29477da553ae194cd6aea03e69f911270c9933566f635c380633bff39ce5',
    'noise_q100_17x33_s2': 'fa211bcff786276e23aa0dfd5b88a663bf6c8fce466e43208fb342dbf731f8df',
    'noise_q100_75x100_s0': 'a73c7f8af09e8846904b069eb14bd36da165da468d082e24b2ee151a8e6c5ffe',
    'noise_q100_75x100_s1': '09e5ce0d1651ad1521fdf4397e6d1ad4de5217c3ee578e9b49664d70fdb896b8',
    'noise_q100_75x100_s2': '635b0a93264fb4219e814038b30a2cfdd13a840158816e8fb9fedb2953efbdc2',
    'noise_q100_8x8_s0': '19bc4ffddf09e09200b7bd8badf41171d0f97d5afa399bf6851a894d0b54dc20',
    'noise_q100_8x8_s1': 'd534dd326b2d1e711ed405a3b41e9b1279e01bf3011703b8193badfb4a8ab0f3',
    'noise_q100_8x8_s2': '1f4ff86f0da501d716e65cbfd1f20761d4c256e9fe382a61c8f939eeadf30444',
    'noise_q100_rstrow_75x100_s2': '7d90d5dbfd95fced3312a0ee145ce8ae5489e4c3b63a97757ae75678d9368dfe',
    'noise_q30_opt_17x33_s0': 'e1c56d5547c7dd6a53bfaca03f2b58fd9026ff3dc3f842c9e61388b6669ad4f3',
    'noise_q30_opt_17x33_s1': 'd685cda2cd682150396a902a8933471355ae9d4af93035d0360a7c1820e427ee',
    'noise_q30_opt_17x33_s2': '20128a0786b2cb3aa47b175b01fe565483218e0b3a22c8418330bcb1b6c404b9',
    'noise_q30_opt_48x64_s0': '6d4614cf8049501fbeaaae61c220b396441c1ad9b2663553af713567de839a1e',
    'noise_q30_opt_48x64_s1': '5af2be54a641798912943e5a288ce92fde4db5db29946904c815ca42c5461116',
    'noise_q30_opt_48x64_s2': 'bb7db589af8354f069b327467c092f02ad38cc5797e36d3a2a03a1c4b52784b3',
    'noise_q30_opt_75x100_s0': '6c9054520d4a490c56151f661a4f23d2df9b80ca46f803eba0fd34c576831dd0',
    'noise_q30_opt_75x100_s1': '1edf71ad9b3d847cd7eb8c7fcb6f7ab7345d35d044fd22fd1a8ef49de8e748ca',
    'noise_q30_opt_75x100_s2': '2579aacbc2220b1ddc9b171894bc46dd160630e404bf1575e7d5432cd521d9a9',
    'noise_q30_opt_7x9_s0': '67d86ddd6398c398c4545a1b5274e5427433fa4cf11bcb29f1972830b66ba309',
    'noise_q30_opt_7x9_s1': 'b982c303c4c2187aa834e6a95d5f68c912153f633aafe9826b1f84d508ce09e7',
    'noise_q30_opt_7x9_s2': 'ded8dc123c85fed6829a9703273a15ba107db178859402b0889b5445fc3d52d8',
    'noise_q30_opt_rst2_75x100_s2': '20d1f0b6f602bb2e76805999eea09bd092c9e63bd617197f5bc1411ec79a730e',
    '*': '3444804181bff06b5f5a466862a1ef64e0e63d6d1954d8849c223e83cb503451',
    'large_file': '3e7510371162cb660b2bba8a4119981c172a205caea3bb1bda9134a0462a9244',
    'orientation6_file': '9d02f1d4a17302aa09509892386dd01200e9e540440e5b9b839395d35409b64d',
}
JPEG_PROGRESSIVE_CASES = {
    'grad_q75_17x33_s0': '14d16d846fb76bdc4be435de0a70864caae984e87536f31a0ba54770a82d14cf',
    'grad_q75_17x33_s1': 'e7ccb2cd62589aa4d3afd33be04e766716e3c277730a4546e56da11ccaf96c1f',
    'grad_q75_17x33_s2': '20020da1dabe9e22850f48f19055be3827bd6283e184c53ee46b5c1ebdd955fe',
    'grad_q75_1x1_s0': '2827e35a54b6d5a45686c5e6f49a0cd7d4edd23337a43554d2e098ee707c6694',
    'grad_q75_1x1_s1': 'e4ab2e7e5187ffca5750f14e9044e6addba7dc1f4c0c9014238c76ac233e2e74',
    'grad_q75_1x1_s2': '642a571b665edbdb8affbd9e244f16a9285a368e2e992db472739e065af3e3f7',
    'grad_q75_48x64_s0': '58def62e63f9537b12eec1e8dfc5f9b38fc8626313503c1a6c7598d48a804b2f',
    'grad_q75_48x64_s1': 'ac600598a73efefa93d8baf42429f7898fb02afeee9b94867a0542a824b6103c',
    'grad_q75_48x64_s2': '8e91232177c7927b4624875da4d628d550b13aab72dfefc65ff6e60c7db5a11e',
    'grad_q75_75x100_s0': 'f39918e19641457b353a16b1ac8d8e337f4cdcbc2a54f18146840697c529bd9c',
    'grad_q75_75x100_s1': 'b657db5f71c89a56f7027a2435b2ff7de47fbb968212b0f4a6e98e016b9f0a67',
    'grad_q75_75x100_s2': '6568a227c19aa0027b4fb43ef5d250a895f580d5a34a34162c09c9d8726ed12f',
    'grad_q75_7x9_s0': '5fbb8665c417db5d529705132cf26f78f477340fdca65f5d47e9714b8aee75d5',
    'grad_q75_7x9_s1': 'd37a4cd3f4b91c9398a0ea818d23347404c64a26e966b94d0b539d4a28a9fbba',
    'grad_q75_7x9_s2': '7e343cd12af2e995b80e7de02095ecf69f7b70f951dc183c52aba34d0c85bc8f',
    'grad_q75_8x8_s0': '19005241662241c8408553f43bef36ab493a92c0fbfa4f7c28558e4446fcd8f3',
    'grad_q75_8x8_s1': '22ec6b003e927acb0a2396cd375248be491658b0a21331dc1f2074cbe4b92ce0',
    'grad_q75_8x8_s2': 'e6e3b535cc2c273167affd0ab3d4d50547be2bd4fe9a374a97bfa2898c7e9a94',
    'grad_q75_rst2_17x33_s0': 'a05115b72d33a722c95e33a6cd5e82a26c62ab199f65d6fa04a62b2f231615ff',
    'grad_q75_rst2_17x33_s1': '3646deef184cce70a675ba968695b5125b0051bcb94f803372f8351508aac351',
    'grad_q75_rst2_17x33_s2': 'e06063414a19a1ba49c44a9537c89383ee37379d220a121d822c6ef093dc2da1',
    'grad_q75_rst2_longeob_17x33_s0': '498dcc4d0d6bd8b7534c0187277eed30fafd43bbb33a655d82ef72d4cca2dfc9',
    'grad_q75_rstrow_48x64_s0': 'a2f2a91c3bde94b26bd064b63f02824cb9b0ec9f8d453a310a154585b75fe0b0',
    'grad_q75_rstrow_48x64_s1': '3aee1e90ce7f3ffa200960ffa59e958b47a02acb90fe92fd96707570052026c8',
    'grad_q75_rstrow_48x64_s2': 'ff6565f721d14ffb03c39aae980be431b3bd7a992bb7bf7b69b35f784a1bd67b',
    'gray_q75_17x33': '89de82da524b7939b4faf5050128d3581e14053138c0d3a45df3efe0b08da79f',
    'noise_q100_17x33_s0': 'b7c63233940ee8878582ba20fc5ad16c3944e6419a231c63a5d7fa2adc907bf1',
    'noise_q100_17x33_s1': '1dfc883348b8e9bce1a465c311d822ecd8d166b3e5348feb609d6b9dc6e5c9e3',
    'noise_q100_17x33_s2': '5996ccd738842d66806f6f0a1bf0539c39253af49360e0afe7a63265d7e58bb7',
    'noise_q100_75x100_s0': 'ac7dd912ae7b08fa807c6aa7845263851fe5a8768b7b47a15be9d0c76be410a8',
    'noise_q100_75x100_s1': 'a5554bd7a81e8edfba1c34deb2d6467b6c108afb934ccdf4133cfe0e6780cfe8',
    'noise_q100_75x100_s2': 'f084d8467bc875864265480313a66ddc41207c0821f998bc0866fc173914399d',
    'noise_q100_8x8_s0': '3293b8214ef0d64ea132d8ee34a99ebb5ef1d7bc185d2b4aec5ffb45d9093292',
    'noise_q100_8x8_s1': 'bf832d29c5151960fb14dc124c48eb49861ea3f8be14630852d9334038fe6b7e',
    'noise_q100_8x8_s2': '6cee98eb251c2bd16b4420afcafaf3f34e5f3616463576c1bb2027ba5e7553ce',
    'noise_q30_opt_17x33_s0': '8f0d00ec3fa138efbe121b99c0343e9802d5a2391acdb92513984b2ec923cb88',
    'noise_q30_opt_17x33_s1': 'ef05ce13ccf6e7973c7a11609701dc911c8b2141ff59424fb654d39a316783ef',
    'noise_q30_opt_17x33_s2': 'c3d33ce09444ee59fd20f8ce54acb3df8fb1716c687251e50a42717d0d7b8ca6',
    'noise_q30_opt_1x1_s0': 'd21c5e1372322f0bccdac58bb8ed5896196de26ece077ab3fddc274a7185e705',
    'noise_q30_opt_1x1_s1': '46bc34702160503ce71d264f286102ba344719ba8c55b63b79dd631d9e3a6f46',
    'noise_q30_opt_1x1_s2': '5ac59da58657ed9acea359d63079479504328f2af31c22debeec8ff1024dff30',
    'noise_q30_opt_48x64_s0': 'ce824524f69d8c4d57391117eae8b903a57329df946ac270de73431439f57a23',
    'noise_q30_opt_48x64_s1': 'c9913b92bd85a99aa55a7cd7466a025d85cf0a2844a24e325db36e543ff668ae',
    'noise_q30_opt_48x64_s2': 'abf537d298dca04121534175a65ac6e3adbf60ace95f3b5feb09adb25c92f4d3',
    'noise_q30_opt_75x100_s0': '6fcd1422fd0b5e889375f7873ed4014202571d2a61029bd1063a95e223848c27',
    'noise_q30_opt_75x100_s1': '48c9918d2d8e7b364a41633c1e6d36969e0a1b8eb1ccba20e0e9b80d4273fd0c',
    'noise_q30_opt_75x100_s2': '673f829ab97b23c6e25d76284890c2f4de8c7922f65c4021b961646b9497d8ad',
    'noise_q30_opt_7x9_s0': '15df6f0a86001c21f925aff77f729fe84fe033050323e05e8d4ec2fcbb6ee0bd',
    'noise_q30_opt_7x9_s1': 'ada6f1724659acc63abcc4307ab138418d3f4f75550456b9be57ea182db62058',
    'noise_q30_opt_7x9_s2': '78ff609dd0c14679d6e951e3f31f049b8eacf7a0defe05783683654df7120de1',
    'noise_q30_opt_8x8_s0': 'bd609f79346842c046fdcd5fdb091cde83c873b4fd6eff8c8c13245877dd6b23',
    'noise_q30_opt_8x8_s1': 'c70c9c3acc990abde14d7fb8b0e5cc2feca1fd5aae2013deb482c01b27feae3b',
    'noise_q30_opt_8x8_s2': 'ea8765f24ab1fdbd20e4c238562b79b09843c391e86200ba8b339c1ceadcdf97',
    'noise_q30_opt_rst2_75x100_s2': 'b5bdc5b3250812136f70280672ae007b62848ed9a8f87952c7003513c237b23e',
    '*': 'cc84bbf2ca6a377b685ddd87fcfa823294b1545a921c0ffbaa3ad0c5bbf046cc',
    'large_file': '171f60517777b860074de0b0b7b40b32f02e3b56577ac50133e7010c95557830',
}
PNG_CASES = {
    'fixed_rgb8_64x48': 'b63223c3e32a0a506368c729689180d994bb1a5cb06e8657a758df12b7c72e12',
    'flat_gray8_64x48': '50042c12235cb2ba0398ac7ce41af9006d28cdd3f614da2f1d024e372bd47411',
    'fullflush_rgb8_64x48': '229c8c1a21236d368af70952ae817199fbef70f4f5d14ead9223d3047a879409',
    'ga16_17x33': '4313df96c85c727a966e992b60ecc19dde4dc27e81e1a91072f2041b60fdc758',
    'ga8_17x33': 'c09f9402957224b0ac99978cad005c934b01665f6253451ad32aa411a1f80a63',
    'gray16_17x33': '59c9f707c281585d7a8e9ca52d04f53ec417fd002ea1ec58e6a9c9a20ecb593d',
    'gray1_17x33': '8648409e47454fdd78e7f668c03a71faf954830f5c4ad590b7ca2383ee80373d',
    'gray1_3x5': '02a8a43113cc6f399240fe61e090d137689f4c4ac0c7b0b9fe44b84e36848f67',
    'gray2_17x33': '5f8b0b8e81a4ad53826ed5ddbe0c986da9c43cc1f81b494195232ed3c6135810',
    'gray2_5x7': 'bf4630744dfba87034f107db86a6f6a996a93b16c311daba569ce1e4f7b7d67d',
    'gray2_filter_cycle_from4_17x33': 'dec6b8f87cc12a210165519513b2b451cf04348458aa08bcb201eb777422661c',
    'gray4_17x33': 'dd02aa686bdb508683a2ae2e8d8dcf385e49074a90ce1c0cb75771ec7443a114',
    'gray4_3x5': 'b9f1feb469e1ff91a8228cbe7685b93a387f2d857d18d255c2580488fe668bd0',
    'gray8_17x33': '9add455296667401fc397f8aa6cc58e02d524a03797c51b08c71b2967a8d721f',
    'gray8_trns_17x33': 'fab3f37939e9a0af35afec0931509bfefffe3d40433160681944055c0eee6e77',
    'huffman_only_rgb8_64x48': 'ed42d3940bb524bfecbfba3d6c91c633d23094482ebecbf43d015cb68e014174',
    'idat1_rgb8_17x33': '095b30469dfff6dffe9f737546fe68cc123ddfcaf72c8734b1c70d93001a2e62',
    'idat7_rgb8_64x48': 'c91aaa57a5c34483c28023c2c42e6cfbf9aa3566d9d4f6860acf6a0e3d5457e9',
    'memlevel1_noise_rgb8_64x48': '755934a232cccc617e75cb0c218cd5fa74b52eab8e3ef3fb310970c7d62233e8',
    'memlevel1_rgb8_64x48': '1fa639e7488519b35a3cc525ff91f1a9e820262ab242fa7344223b917c950b2f',
    'pal1_17x33': 'f633347e75216f77b181d2af39bac00ed8d4e47c8494b6a10208b9c99a3fa01b',
    'pal2_5x7': 'eded405dd00e887e04ada8b260a2d0c93aeff8cb32141852d0a61e08f0e4ea79',
    'pal4_17x33': 'acdab1491d8f5b42846b8e7720a560499f8a4d191ae58d379a67723cba10528f',
    'pal4_3x5': '075da5b3247b64bfeece3b2ee34cab73cdf51514a3afeb154c6c445dea6deffd',
    'pal4_short_plte_17x33': '02fb4055271d8e07bce7c393d8fc2cc9bdc26976cd339f27324100305bffb2bc',
    'pal8_17x33': '04f99b69ab027a052a697418503bf48ee5ce5fce63f7bac9d389a8be84894593',
    'pal8_trns_17x33': 'ab35ff5296a72de8448317ff53a24e68ba4847ff94c9087c19d8bb64603ec07a',
    'rgb16_17x33': 'daf791c70508e97bddc884be2a14dd55c6c761125f784d7fc5f8241517b9da94',
    'rgb8_17x33': '1830f488522ca14bb02556060bc65b317dd4075c8d9fcb23532e8a13cd3d170e',
    'rgb8_1x1': '36f1db6f3e5c1df775cc79290d725b633fa32fb4ef8f1cb213e5b1d3363a01d9',
    'rgb8_1x7': 'd95d1839221f9a6f6192756995ba848c943dfed35192146ac30d426647a70fc8',
    'rgb8_3x5': '4a5f61abb4e9837393586b76cbe578e0aa2f901d2e7a5b09d6b4943fceb24f59',
    'rgb8_64x48': '23a33bf13f3d837418bc2bed26583c7f001ae53f527f5896f72fd03deaaacfd8',
    'rgb8_7x1': 'c7995236fe9341252da443acf7b7c7415b17c7fbef19540377ef0fba8ea98084',
    'rgb8_filter0_17x33': '8976c9d492a66f0fc5e83e4dd7645f99c87cbbc093ca0386b4fe47ad86f426d8',
    'rgb8_filter1_17x33': 'e9fbb1f1e394bbd90229d0cb809474a2df40ba5a42c5983ee517221840e3c8f6',
    'rgb8_filter2_17x33': '4ceefab76593f64ca01bcbfb1d4fa1cf172e6b7fe3e7dc9bf0136d9939d0db08',
    'rgb8_filter3_17x33': '1cee6ddd1b976b1aa7cbdab75f847073bb38769b919caf5d44702d3197611a29',
    'rgb8_filter4_17x33': 'f685a586249e81b9dde7b7140a0e766a0c013bde4bbb2c9b5016675c885a3dd2',
    'rgb8_trns_anc_17x33': 'ae281a2b45ebc25b3615c84c63ea69bda7bddd1b4d21463a6d66ee489782d1b1',
    'rgba16_17x33': '45171a95520e168c45d630e221ce9bfa0d66aabc2d52f749dcdc0d15b79119b3',
    'rgba16_filter0_5x7': '1837ec0d6fef931a23df2431763f4fa2bcd4298738168bd99942737bf937fd14',
    'rgba16_filter1_5x7': 'dda162c1d2f9e376fe4c9a4ad1088eec0b002c6e78b862c092986fa019804e10',
    'rgba16_filter2_5x7': '66f24bbcc3eb1996e19e507be18602fef3744d559e311a5a895899df89d77f10',
    'rgba16_filter3_5x7': 'ad37d941e8d7c67e0d328724073ff21e37a19c615c5ba89f05b2d097ce06ff48',
    'rgba16_filter4_5x7': 'c48340e6a1642ee478e6efceba01f6b46e0dfcacc4e3e22015c8b2542adf96d1',
    'rgba8_17x33': '705fc4a34b583c466033f5ae167c9d7bd410affe03487945bccd06d7a6398d99',
    'rle_rgb8_64x48': 'bc8a772af2a210f771427cc38e479c0ed63ecf57c5c453a758dffe8e3cece532',
    'stored_rgb8_64x48': '213df9ad83b2fad3a2a546186e3476bda93628eaf64833e7ffcebcac3a18ddcc',
    'stored_straddle_rgba16_128x100': 'aa175728608839935e9d5652027b86354b3c9fbd1cee908b3a0d66be70abb935',
    'window_rgb8_128x100': '81fdd3b85a5daa55eec1d3527eb58b29ad82f289aa5b36d9c0c6854ee2e4d4b6',
    '*': '1742fba8ce71dc41f7ec30e3c85dd9f8e446519cb3487f3d589444b84696d4d7',
    'badfile_distance_before_start': 'd9ee3cba86f0c209136bda5f1e6bf50e8a0a62acece641a3cc2a69cca216b615',
    'badfile_filter_byte_7': '0908035459513541042eac16cafbade3cf06603b07ec202c2c22834aee10e5aa',
    'badfile_idat_cut_to_half': '75ee8ef3cee58f72c76eaff859a77c6db4ca3c917810e25b40b2325573f213e7',
    'badfile_palette_index_past_plte': 'd67dcf6aadd5a1532e8ecd4697baef1e6f380ee4e8497d6b9101f53d52d69d06',
}


def _jpeg_digest(datas, progressive):
    infos = [J.parse(d, progressive) for d in datas]
    hdr, images, lanes, huff, quant, scan_at, prog = J.build_blob(datas, infos)
    buf = np.zeros(int(hdr["total_bytes"]), np.uint8)
    J.fill_blob(buf, hdr, images, lanes, huff, quant, datas, infos, scan_at, prog)
    return hashlib.sha256(buf.tobytes()).hexdigest()


def _png_digest(datas):
    infos = [P.parse(d) for d in datas]
    hdr, images, palette = P.build_blob(infos)
    buf = np.zeros(int(hdr["total_bytes"]), np.uint8)
    P.fill_blob(buf, hdr, images, palette, datas, infos)
    return hashlib.sha256(buf.tobytes()).hexdigest()


@pytest.mark.parametrize("name, want, digest", [("jpeg_cases", JPEG_CASES, lambda ds: _jpeg_digest(ds, False)),
                                                ("jpeg_progressive_cases", JPEG_PROGRESSIVE_CASES, lambda ds: _jpeg_digest(ds, True)),
                                                ("png_cases", PNG_CASES, _png_digest)], ids=["jpeg", "jpeg_progressive", "png"])
def test_blob_bytes_are_those_of_the_hand_written_layouts(golden, name, want, digest):
    z = golden(name)
    names = sorted(k[5:] for k in z.files if k.startswith("file_"))
    assert set(names) | {"*"} <= set(want)                    # every file_* entry of the set, and the set as one call
    for k, sha in want.items():
        datas = [z["file_" + n].tobytes() for n in names] if k == "*" else [z[k if "file" in k else "file_" + k].tobytes()]
        assert digest(datas) == sha, k


def test_layout_offsets_are_aligned_ordered_and_disjoint():
    dt = np.dtype([("a", "<i8"), ("b", "<i8"), ("c", "<i8"), ("d", "<i8"), ("e", "<i8"), ("n", "<i4")])      # 44 bytes: not a multiple of 16
    sizes = (0, 1, 15, 16, 17)
    sections = [(f, np.arange(n, dtype=np.uint8)) for f, n in zip("abcde", sizes)]
    hdr, total = S.blob_layout(dt, sections)
    offs = [int(hdr[f]) for f in "abcde"]
    assert offs == [48, 48, 64, 80, 96] and total == 128 and int(hdr["n"]) == 0
    end = dt.itemsize
    for o, n in zip(offs, sizes):
        assert o % 16 == 0 and o >= end
        end = o + n
    assert total == S.align(end) and total % 16 == 0
    assert [S.align(x) for x in (0, 1, 15, 16, 17)] == [0, 16, 16, 16, 32] and S.align(9, 8) == 16


def test_writer_round_trips():
    dt = np.dtype([("x_off", "<i8"), ("y_off", "<i8"), ("z_off", "<i8"), ("count", "<i4")])
    rng = np.random.default_rng(0)
    sections = [("x_off", rng.integers(0, 1 << 15, (3, 7), np.int64).astype(np.uint16)), ("y_off", np.zeros(0, np.int32)),
                ("z_off", rng.integers(0, 255, 17, np.int64).astype(np.uint8))]
    hdr, total = S.blob_layout(dt, sections)
    hdr["count"] = 3
    buf = np.full(total, 0xEE, np.uint8)
    S.write_blob(buf, hdr, sections)
    assert np.array_equal(np.frombuffer(buf[:dt.itemsize].tobytes(), dt)[0], hdr)
    used = np.zeros(total, bool)
    used[:dt.itemsize] = True
    for f, arr in sections:
        o = int(hdr[f])
        assert np.array_equal(np.frombuffer(buf[o:o + arr.nbytes].tobytes(), arr.dtype).reshape(arr.shape), arr)
        used[o:o + arr.nbytes] = True
    assert (buf[~used] == 0xEE).all()                          # the gaps are the caller's


class _Library:
    """A stand-in for the HIP library: one maf_*_struct_sizes export, counting its calls."""

    def __init__(self, sizes):
        self.sizes, self.calls = sizes, 0

    def maf_fake_struct_sizes(self, out):
        self.calls += 1
        out[:] = self.sizes
        return 0


def test_checked_library_checks_once_per_key_and_again_after_a_failure(monkeypatch):
    fake = _Library([40, 24])
    monkeypatch.setattr(S.lib, "load", lambda: fake)
    monkeypatch.setattr(S, "_checked", set())
    args = ((("maf_fake_struct_sizes", 2),), [40, 24], "maf_fake_* structs")
    assert S.checked_library("fake", *args) is fake and S.checked_library("fake", *args) is fake
    assert fake.calls == 1
    fake.sizes = [40, 25]                                      # one byte too many
    with pytest.raises(MafError, match=r"built for maf_fake_\* structs of \[40, 25\] bytes, this binding declares \[40, 24\]: rebuild"):
        S.checked_library("other", *args)
    with pytest.raises(MafError, match="rebuild"):
        S.checked_library("other", *args)                       # a failure is not remembered
    assert fake.calls == 3
    fake.sizes = [40, 24]
    assert S.checked_library("other", *args) is fake and S.checked_library("other", *args) is fake
    assert fake.calls == 4
    one = _Library([72])                                        # a bare int: the size itself in the message
    monkeypatch.setattr(S.lib, "load", lambda: one)
    with pytest.raises(MafError, match="built for a maf_fake_t of 72 bytes, this binding declares 71: rebuild"):
        S.checked_library("one", (("maf_fake_struct_sizes", 1),), 71, "a maf_fake_t")


def test_file_bytes_file_name_and_status_text(tmp_path):
    data = b"\xff\xd8 not much of a file"
    p = tmp_path / "a file.jpg"
    p.write_bytes(data)
    for src in (p, str(p), data, bytearray(data), memoryview(data)):
        got = S.file_bytes(src)
        assert type(got) is bytes and got == data
    assert J._bytes is S.file_bytes and P.file_bytes is S.file_bytes
    assert S.file_name(p, 3) == "file 3 (%s)" % p and S.file_name(str(p), 0) == "file 0 (%s)" % p
    assert S.file_name(pathlib.PurePosixPath("d/x.png"), 12) == "file 12 (d/x.png)"
    for src in (data, bytearray(data), memoryview(data)):
        assert S.file_name(src, 7) == "file 7"
    two = J.STATUS_BAD_CODE | J.STATUS_SHORT_SCAN
    assert J.status_text(two) == S.status_text(J._STATUS_TEXT, two) == "an invalid Huffman code, a scan that ends early"
    assert J.status_text(1 << 20) == "status 0x100000" and J.status_text(two | 1 << 20) == J.status_text(two)
    assert P.status_text(P.STATUS_BAD_FILTER | P.STATUS_BAD_PALETTE_INDEX) == "a filter type above 4, a palette index past PLTE"
    assert P.status_text(1 << 20) == "status 0x100000" and J.status_text(0) == "status 0x0"


def test_raise_on_status_words_the_two_decoders_ways():
    files = [b"", "b.png", b""]
    S.raise_on_status("x.decode", files, [0, 0, 0], P._STATUS_TEXT, True)
    with pytest.raises(MafError) as e:
        S.raise_on_status("png.decode", files, [0, 256, 1], P._STATUS_TEXT, True)
    assert str(e.value) == "png.decode: file 1 (b.png): a filter type above 4 (status 0x100); file 2: a deflate stream that ends early (status 0x1)"
    with pytest.raises(MafError) as e:
        S.raise_on_status("jpeg.decode", files, [4, 0, 0], J._STATUS_TEXT, False)
    assert str(e.value) == "jpeg.decode: file 0: a scan that ends early"


def test_frame_list_on_the_host_in_both_wordings():
    cpu = torch.zeros(4, 5, 3, dtype=torch.uint8)
    for frames in ([cpu], cpu[None]):
        with pytest.raises(MafError) as e:
            S.frame_list(frames, LB._FRAME_TEXT, "resize_area")
        assert str(e.value) == "resize_area runs on the HIP path only: frames must be CUDA tensors (no CPU fallback)"
        with pytest.raises(MafError) as e:
            S.frame_list(frames, E._FRAME_TEXT)
        assert str(e.value) == "jpeg_encode.encode runs on the HIP path only (no CPU fallback): frame 0 is on cpu"
    with pytest.raises(MafError, match="^eval_batch runs on the HIP path only: frames must be CUDA tensors"):
        S.frame_list([np.zeros((4, 5, 3), np.uint8)], LB._FRAME_TEXT, "eval_batch")
    with pytest.raises(MafError, match="^jpeg_encode.encode: frame 0 is a ndarray, not a CUDA tensor$"):
        S.frame_list([np.zeros((4, 5, 3), np.uint8)], E._FRAME_TEXT)
    with pytest.raises(MafError, match="^letterbox: no frames$"):
        S.frame_list([], LB._FRAME_TEXT, "letterbox")
    with pytest.raises(MafError, match="^jpeg_encode.encode: no frames$"):
        S.frame_list((), E._FRAME_TEXT)
    with pytest.raises(MafError, match=r"^letterbox: a single tensor of frames is uint8 \[B, h, w, 3\]$"):
        S.frame_list(cpu, LB._FRAME_TEXT, "letterbox")
    with pytest.raises(MafError, match=r"^jpeg_encode.encode: a tensor of frames is \[B, h, w, 3\], got \(4, 5, 3\)$"):
        S.frame_list(cpu, E._FRAME_TEXT)


def test_cuda_device_refuses_the_host():
    with pytest.raises(MafError, match=r"^png.decode runs on the HIP path only \(no CPU fallback\): device cpu$"):
        S.cuda_device("cpu", "png.decode")
