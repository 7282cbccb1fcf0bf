"""One match_keywords.run over WORK/articles.csv in a process of its own (tests/test_gpu_stamps_e2e.py).

The process's time zone is its environment's TZ from the start, as a user's is; the knowledge base is the golden
one.  Usage, from the repository root:

    TZ=EST5EDT,M3.2.0,M11.1.0 KW_STAMPS_NATIVE=1 python -m tests.stamps_e2e_worker WORK

writes WORK/yahoo_ticker_matched_articles/ and prints one JSON line."""
import json
import os
import sys


def main(work):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import advanced_scrapper_amd
    from advanced_scrapper_amd import _native, ingest, match_keywords as mk
    from tests import golden_data
    # the package and its libraries are this tree's
    assert os.path.dirname(os.path.dirname(os.path.abspath(advanced_scrapper_amd.__file__))) == repo
    assert os.path.dirname(os.path.dirname(os.path.dirname(_native.DEFAULT_LIB))) == repo
    os.chdir(work)
    mk.read_and_process_json_files = lambda _d: golden_data.kb_processed()
    args = mk._parse(['--info-dir', 'unused', '--articles', os.path.join(work, 'articles.csv'), '--chunksize', '128'])
    rc = mk.run(args, 0, 1, None, None)
    st = ingest.LAST_STATS or {}
    print(json.dumps({'rc': rc, 'tz': os.environ.get('TZ'), 'stamps_slow': st.get('stamps_slow'),
                      'dates_slow': st.get('dates_slow'), 'routes': st.get('routes'),
                      'stamps_ms': st.get('stamps_ms'), 'lib': _native.LIB_PATH}))


if __name__ == '__main__':
    main(sys.argv[1])
