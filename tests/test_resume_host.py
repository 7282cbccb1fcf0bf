"""CPU: the pandas route of resume.remaining_urls (KW_RESUME_NATIVE=0) against a direct restatement of
constant_rate_scrapper.py:312-360."""
import csv
import os

import pandas as pd
import pytest

from advanced_scrapper_amd import resume

SUCCESS = resume.SUCCESS_FIELDS
FAILED = resume.FAILED_FIELDS


def reference_lines(links='yfin_urls.csv', website='yfin'):
    """:312-360: (initial_total, scraped_success, scraped_fails, urls, printed lines)."""
    df_links = pd.read_csv(links)
    all_urls = df_links["url"].astype(str).tolist()
    initial_total = len(all_urls)
    scraped_urls = set()
    scraped_success = scraped_fails = 0
    if os.path.exists(f"success_articles_{website}.csv"):
        df = pd.read_csv(f"success_articles_{website}.csv")
        scraped_success = len(df)
        scraped_urls.update(df["url"].astype(str).tolist())
    if os.path.exists(f"failed_articles_{website}.csv"):
        df = pd.read_csv(f"failed_articles_{website}.csv")
        scraped_fails = len(df)
        scraped_urls.update(df["url"].astype(str).tolist())
    df_links = df_links[~df_links["url"].astype(str).isin(scraped_urls)]
    urls = df_links["url"].astype(str).tolist()
    lines = [f"Total URLs in CSV: {initial_total}", f"Already scraped (Success + Fails): {scraped_success + scraped_fails}",
             f"Remaining URLs to scrape: {len(urls)}"]
    return initial_total, scraped_success, scraped_fails, urls, lines


def write_files(links, success=None, failed=None, website='yfin'):
    pd.DataFrame({'date_time': range(len(links)), 'url': links}).to_csv('yfin_urls.csv', index=False)
    for name, fields, rows in ((f'success_articles_{website}.csv', SUCCESS, success),
                               (f'failed_articles_{website}.csv', FAILED, failed)):
        if rows is None:
            continue
        with open(name, 'w', newline='', encoding='utf-8') as fh:
            w = csv.DictWriter(fh, fieldnames=fields)
            w.writeheader()
            for u in rows:
                row = {f: 'x' for f in fields}
                row['url'] = u
                if 'article' in row:
                    row['article'] = 'Line one.\n"Quoted, text"\r\nhttp://l/3 in the text'
                w.writerow(row)


def check(capsys, **kw):
    want = reference_lines(website=kw.get('website', 'yfin'))
    capsys.readouterr()
    got = resume.remaining_urls(**kw)
    out = capsys.readouterr().out.splitlines()
    assert (got.initial_total, got.scraped_success, got.scraped_fails, got.urls()) == want[:4]
    assert got.remaining == len(want[3]) and out == want[4] and got.route == 'pandas'
    b, off = got.arrays()
    assert [b.tobytes()[off[k]:off[k + 1]].decode() for k in range(len(off) - 1)] == want[3]
    got.write('remaining.txt')
    assert open('remaining.txt', 'rb').read() == ''.join(u + '\n' for u in want[3]).encode()
    return got


@pytest.fixture()
def cwd(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('KW_RESUME_NATIVE', '0')
    return tmp_path


def test_both_files_and_duplicate_links(cwd, capsys):
    links = ['http://l/%d' % (k % 7) for k in range(20)] + ['http://l/x,y', 'http://l/é']
    write_files(links, success=['http://l/1', 'http://l/1', 'http://other/'], failed=['http://l/3', 'http://l/x,y'])
    got = check(capsys)
    assert got.initial_total == 22 and got.scraped_success == 3 and got.scraped_fails == 2
    assert got.urls().count('http://l/0') == 3 and 'http://l/1' not in got.urls()   # rows, not unique URLs


def test_missing_success_or_failed_file(cwd, capsys):
    links = ['http://l/%d' % k for k in range(5)]
    write_files(links)
    assert check(capsys).remaining == 5
    write_files(links, failed=['http://l/2'])
    got = check(capsys)
    assert (got.scraped_success, got.scraped_fails, got.remaining) == (0, 1, 4)
    os.remove('failed_articles_yfin.csv')
    write_files(links, success=links)
    got = check(capsys)
    assert (got.scraped_success, got.scraped_fails, got.remaining) == (5, 0, 0) and got.urls() == []


def test_other_website_and_paths(cwd, capsys):
    write_files(['http://l/1', 'http://l/2'], failed=['http://l/2'], website='abc')
    assert check(capsys, website='abc').urls() == ['http://l/1']
    got = resume.remaining_urls(links_csv=str(cwd / 'yfin_urls.csv'), failed_csv=str(cwd / 'failed_articles_abc.csv'))
    assert got.urls() == ['http://l/1']


def test_missing_links_file_raises_what_pandas_raises(cwd):
    with pytest.raises(FileNotFoundError) as want:
        pd.read_csv('yfin_urls.csv')
    with pytest.raises(FileNotFoundError) as got:
        resume.remaining_urls()
    assert str(got.value) == str(want.value)
