"""cdx_dedup.merge_parts without any readable part: the reference's messages, on either route, with no GPU."""
import os

import pytest

from advanced_scrapper_amd import cdx_dedup


@pytest.mark.parametrize('native', ['unset', '0'])
def test_merge_without_readable_parts_needs_no_gpu(tmp_path, monkeypatch, capsys, native):
    def no_gpu():
        raise AssertionError('the dedup handle was asked for')
    monkeypatch.setattr(cdx_dedup, '_dedup', no_gpu)
    if native == 'unset':
        monkeypatch.delenv('KW_CDX_NATIVE', raising=False)
    else:
        monkeypatch.setenv('KW_CDX_NATIVE', native)
    assert cdx_dedup.native_enabled() == (native == 'unset')
    d = tmp_path / 'parts'
    os.makedirs(d)
    out = tmp_path / 'yfin_urls.csv'
    assert cdx_dedup.merge_parts(str(d), str(out)) is None
    assert capsys.readouterr().out == "No CSV files were processed. Check if the scraping was successful.\n"
    (d / 'yahoo_AA.csv').write_bytes(b'')
    assert cdx_dedup.merge_parts(str(d), str(out)) is None
    assert capsys.readouterr().out == (f"Error reading {d / 'yahoo_AA.csv'}: No columns to parse from file\n"
                                       "No CSV files were processed. Check if the scraping was successful.\n")
    assert not out.exists()
